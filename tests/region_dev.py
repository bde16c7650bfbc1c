"""Device helpers of the region-map GPU suites: arrays to and from cuda:0, the
word-guarded output buffer and its checked head, and the key-by-key comparison
with a model.  torch is imported inside the functions, so a machine without it
can still import the modules that use these."""
import numpy as np

SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}      # torch storage by item size


def to_dev(a, dtype=None):
    """A contiguous copy of `a` (cast to `dtype` first, if given) on cuda:0, as the torch dtype of its item size."""
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(SIGNED[a.dtype.itemsize]).copy()).to("cuda:0")


def to_host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def guarded(count, guard, fill):
    """An int32 tensor of `count` + `guard` words, every one the 32-bit pattern `fill`."""
    import torch
    return torch.full((count + guard,), int(np.array(fill, np.uint32).view(np.int32)), dtype=torch.int32,
                      device="cuda:0")


def body(t, count, guard, fill, what):
    """The first `count` words of a guarded tensor; it has `guard` more, and they are intact."""
    a = to_host(t)
    assert a.size == count + guard and (a[count:] == fill).all(), "guard words of %s" % what
    return a[:count]


def same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), k
