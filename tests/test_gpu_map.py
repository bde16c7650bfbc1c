"""GPU: map_colors_mps alone, where its exactness arguments are thin.

The map's answer is the argmin over (squared distance, MPS visit rank); the
cell build drops entries with two filters that must never drop one that can
win or TIE.  Uniformly random pixels almost never tie, so these tests map
pixels built from the palette itself (fx.map_probe_pixels: entries, pair
midpoints, cell corners, garbage top bytes -- on the lattice palettes 3 in 4
midpoints are exact ties, up to 8-way) and all 2^24 colours, on palettes at
the candidate-count thresholds (3 compact inline, 7 inline, 32 per-cell cap)
and up to the ABI's 16384 entries, through both map kernels
(map_lds_kernel; map_kernel, which palettes above 1024 entries and misaligned
buffers take anyway), at ragged and tiny sizes, from misaligned buffers and
in sequences of calls on one engine.

References: tests/golden/map2.json (the reference build's outputs, made by
tests/golden/make_golden.py --only map2) and the CPU oracle's literal walk
dqo_map, which test_oracle_golden.py pins to that file.  Every output buffer
starts as a sentinel no palette holds (its top byte is set), so a kernel that
did not run cannot pass.
"""
import ctypes
import functools

import numpy as np
import pytest

import dq_fixtures as fx

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
MAP2 = fx.load_json("map2.json")
MAP2_IDS = ["%s%d" % (c["spec"]["kind"], c["spec"]["k"]) for c in MAP2["palettes"]]
LATTICE32, LATTICE16, CUBE10 = 0, 1, 2      # indices into map2_palette_specs()


@pytest.fixture(params=[True, False], ids=["lds", "gather"])
def mappath(gpu, request):
    """Both map kernels for palettes of at most 1024 entries: map_lds_kernel
    and map_kernel<false>."""
    gpu.set_lds_map(request.param)
    try:
        yield request.param
    finally:
        gpu.set_lds_map(True)


def _oracle_map(px, pal):
    px = np.ascontiguousarray(px, np.uint32)
    pal = np.ascontiguousarray(pal, np.uint32)
    out = np.zeros(len(px), np.uint32)
    fx.oracle().dqo_map(fx.vp(px), ctypes.c_uint32(len(px)), fx.vp(out), fx.vp(pal), ctypes.c_int(len(pal)))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _map2_case(i):
    """(palette, probe pixels, the oracle's outputs) of map2 palette i; computed once, read-only."""
    spec = fx.map2_palette_specs()[i]
    pal = fx.make_palette(spec)
    px = fx.map_probe_pixels(pal, fx.map2_seed(spec))
    pal.setflags(write=False)
    px.setflags(write=False)
    return pal, px, _oracle_map(px, pal)


@functools.lru_cache(maxsize=None)
def _random_case(k, n=None):
    """The `random` palette of k entries (the map.json spec) on its probe pixels, repeated up to n."""
    spec = {"k": k, "kind": "random", "seed": 77 + k}
    pal = fx.make_palette(spec)
    px = fx.map_probe_pixels(pal, fx.map2_seed(spec))
    if n is not None:   # (from its last two entries on: entries, then midpoints)
        px = np.resize(px[max(0, k - 2):], n)
    pal.setflags(write=False)
    px.setflags(write=False)
    return pal, px, _oracle_map(px, pal)


@functools.lru_cache(maxsize=None)
def _cube_case(i):
    """(palette, the oracle's outputs) of cube palette i over all 2^24 colours."""
    pal = fx.make_palette(fx.map2_cube_specs()[i])
    return pal, _oracle_map(np.arange(1 << 24, dtype=np.uint32), pal)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to("cuda:0")   # (a copy: inputs are read-only)


def _sentinel(n):
    import torch
    return torch.full((n,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _map_dev(gpu, px, pal):
    import torch
    t_in = _dev(px)
    t_out = _sentinel(len(px))
    gpu.map_device(t_in, t_out, pal)
    torch.cuda.synchronize()
    return _host(t_out)


def _explain(px, pal, got, want):
    """The first differing pixel, with the distances that decide it."""
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return "outputs equal"
    i = int(bad[0])
    p = int(px[i]) & 0xFFFFFF

    def d2(c):
        return sum((((p >> s) & 0xFF) - ((int(c) >> s) & 0xFF)) ** 2 for s in (16, 8, 0))

    dist = np.array([d2(c) for c in np.asarray(pal) & 0xFFFFFF])
    dmin = int(dist.min())
    ties = sorted({"%06x" % (int(c) & 0xFFFFFF) for c in np.asarray(pal)[dist == dmin]})
    if int(got[i]) == SENTINEL:
        g = "the sentinel (never written)"
    else:
        g = "%06x at d2 %d" % (int(got[i]), d2(got[i]))
    return ("K=%d: %d of %d pixels differ (%d still the sentinel); first at %d: pixel %08x -> %s, oracle %06x at d2 %d; "
            "minimum d2 %d held by %d colour(s) %s"
            % (len(pal), len(bad), len(px), int((got == SENTINEL).sum()), i, int(px[i]), g, int(want[i]),
               d2(want[i]), dmin, len(ties), ties[:8]))


def _check(gpu, px, pal, want, what=""):
    got = _map_dev(gpu, px, pal)
    assert np.array_equal(got, want), "%s %s" % (what, _explain(px, pal, got, want))


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(MAP2["palettes"])), ids=MAP2_IDS)
def test_map2_fixtures(gpu, mappath, i):
    """Every map2.json palette on its tie-dense probe pixels, against the
    reference's output hash."""
    c = MAP2["palettes"][i]
    assert c["spec"] == fx.map2_palette_specs()[i]
    pal, px, want = _map2_case(i)
    assert len(px) == c["n_px"]
    got = _map_dev(gpu, px, pal)
    if "%016x" % fx.fnv(got) != c["out_fnv"]:
        pytest.fail("%s: %s" % (c["spec"], _explain(px, pal, got, want)))
    assert [int(v) for v in got[:64]] == c["first"]


@pytest.mark.parametrize("i", range(len(MAP2["cubes"])), ids=["subdivided125", "random16"])
def test_map_full_cube(gpu, mappath, i):
    """All 2^24 colours: every colour of every cell against both elimination
    filters of the cell build."""
    import torch
    c = MAP2["cubes"][i]
    assert c["spec"] == fx.map2_cube_specs()[i]
    pal, want = _cube_case(i)
    assert "%016x" % fx.fnv(want) == c["out_fnv"]
    t_in = torch.arange(1 << 24, dtype=torch.int32, device="cuda:0")
    t_out = _sentinel(1 << 24)
    gpu.map_device(t_in, t_out, pal)
    torch.cuda.synchronize()
    t_want = _dev(want)
    if not torch.equal(t_out, t_want):
        pytest.fail(_explain(np.arange(1 << 24, dtype=np.uint32), pal, _host(t_out), want))
    assert "%016x" % fx.fnv(_host(t_out)) == c["out_fnv"]


@pytest.mark.parametrize("k", [1, 2, 512, 4096])
def test_map_small_and_ragged(gpu, mappath, k):
    """Fewer pixels than one 8-pixel group, one group, a group and a tail, and
    ragged sizes of a few workgroups: slices of the lattice (step 32) probe
    pixels that straddle its entries and its midpoints."""
    px_all = _map2_case(LATTICE32)[1]
    if k == 512:
        pal, _, want_all = _map2_case(LATTICE32)
    else:
        pal = _map2_case(LATTICE16)[0] if k == 4096 else _random_case(k)[0]
        want_all = _oracle_map(px_all, pal)
    assert len(pal) == k
    for n in (1, 5, 7, 8, 9, 15, 8197, 16389):
        off = 500 + n % 7
        _check(gpu, px_all[off:off + n], pal, want_all[off:off + n], "n=%d" % n)


def test_map_many_iterations(gpu):
    """map_lds_kernel with more groups per workgroup than its 1024 lanes: a
    second, partial iteration of the prefetch pipeline, then the tail.  A
    block of 8 x 7501 probe pixels repeated to 3000005: the expected output
    is the oracle's block, repeated (8 | block: the repeats stay aligned)."""
    import torch
    pal, px, _ = _map2_case(LATTICE32)
    blk = np.resize(px, 8 * 7501)
    ref = _oracle_map(blk, pal)
    n = 3000005
    reps = (n + len(blk) - 1) // len(blk)
    t_in = _dev(blk).repeat(reps)[:n].contiguous()
    t_out = _sentinel(n)
    gpu.set_lds_map(True)
    gpu.map_device(t_in, t_out, pal)
    torch.cuda.synchronize()
    t_ref = _dev(ref)
    full = n // len(blk)
    head = t_out[:full * len(blk)].view(full, -1)
    if not bool((head == t_ref).all()) or not torch.equal(t_out[full * len(blk):], t_ref[:n - full * len(blk)]):
        pytest.fail(_explain(np.resize(blk, n), pal, _host(t_out), np.resize(ref, n)))


@pytest.mark.parametrize("k", [16, 2000])
@pytest.mark.parametrize("n", [5, 70001])
def test_map_misaligned(gpu, mappath, n, k):
    """Input and / or output 4-B but not 16-B aligned (the staged path), then
    an aligned call on the same engine; nothing is written outside the
    output's n words."""
    import torch
    pal, px, want = _random_case(k, n)
    pad = 8
    for off_in, off_out in ((1, 0), (0, 1), (3, 2)):
        base_in = _sentinel(n + 2 * pad)
        base_in[off_in:off_in + n] = _dev(px)
        base_out = _sentinel(n + 2 * pad)
        t_in, t_out = base_in[off_in:off_in + n], base_out[off_out:off_out + n]
        assert t_in.data_ptr() % 16 == 4 * off_in and t_out.data_ptr() % 16 == 4 * off_out
        gpu.map_device(t_in, t_out, pal)
        torch.cuda.synchronize()
        got = _host(base_out)
        assert np.array_equal(got[off_out:off_out + n], want), \
            "offsets (%d, %d): %s" % (off_in, off_out, _explain(px, pal, got[off_out:off_out + n], want))
        assert (got[:off_out] == SENTINEL).all() and (got[off_out + n:] == SENTINEL).all(), (off_in, off_out)
    _check(gpu, px, pal, want, "aligned after staged")


def test_map_call_sequence(gpu):
    """One engine, calls in a row: the largest palette, a tiny one, the LDS
    kernel's largest, the largest again, a staged call, one entry.  Each call
    finds the previous call's cell tables, palette staging and LDS limits."""
    import torch
    specs = fx.map2_palette_specs()
    big = specs.index({"k": 16384, "kind": "random", "seed": 77 + 16384})
    big2 = specs.index({"k": 16384, "kind": "sametsum", "seed": 91 + 16384})
    tiny = specs.index({"k": 3, "kind": "cluster", "seed": 303})
    gpu.set_lds_map(True)
    for step, case in enumerate([_map2_case(big), _map2_case(tiny), _random_case(1024), _map2_case(big2),
                                 "staged", _random_case(1)]):
        if case == "staged":
            pal, px, want = _random_case(2000)
            base_in = _sentinel(len(px) + 4)
            base_in[1:1 + len(px)] = _dev(px)
            t_out = _sentinel(len(px))
            gpu.map_device(base_in[1:1 + len(px)], t_out, pal)
            torch.cuda.synchronize()
            got = _host(t_out)
            assert np.array_equal(got, want), "step %d (staged): %s" % (step, _explain(px, pal, got, want))
        else:
            pal, px, want = case
            _check(gpu, px, pal, want, "step %d" % step)


@pytest.mark.parametrize("i", [LATTICE32, CUBE10], ids=["lattice512", "cube1000"])
def test_map_bgr24_probe(gpu, i):
    """The probe pixels as BGR24 bytes (n = 5 mod 8: whole 24-byte groups and a
    byte-wise tail) from an 8-B aligned base (read directly by map_lds_kernel)
    and from a base 3 bytes in (packed first)."""
    import torch
    pal, px, want = _map2_case(i)
    n = len(px)
    assert n % 8 == 5
    p = px & np.uint32(0xFFFFFF)
    bgr = np.stack([p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF], -1).astype(np.uint8).reshape(-1)
    raw = torch.full((3 * n + 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    gpu.set_lds_map(True)
    for off in (0, 3):
        raw[off:off + 3 * n] = torch.from_numpy(bgr).to("cuda:0")
        d_bgr = raw[off:off + 3 * n]
        assert d_bgr.data_ptr() % 8 == off
        t_out = _sentinel(n)
        gpu.map_bgr24_device(d_bgr, n, 1, t_out, pal)
        torch.cuda.synchronize()
        got = _host(t_out)
        assert np.array_equal(got, want), "base + %d: %s" % (off, _explain(p, pal, got, want))
