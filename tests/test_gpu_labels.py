"""GPU: per-pixel cluster labels (u8 / u16 / u32 label maps).

The label of a pixel is the lowest index i with ct[i] == the colour the
colour map writes for it (low 24 bits).  Expected labels come from the CPU
oracle's literal walk dqo_map (test_oracle_golden.py pins it to the reference
build's map2.json), converted with that rule; every test also asserts
pal[labels] == the oracle's colours.  Every label buffer starts as 0xA5 bytes
between two guard zones of 0xA5 bytes that must still be 0xA5 afterwards.

Map cases run through both map kernels where the palette allows it
(map_lds_kernel and map_kernel<false> for K <= 1024; above that map_kernel<true>
in any case); the quant cases compare against the reference build's outputs in
tests/golden/ (ct[labels] hashes to the fixture's out_fnv)."""
import ctypes
import functools

import numpy as np
import pytest

import dq_fixtures as fx

pytestmark = pytest.mark.gpu

GUARD = 64                     # bytes before and after every label buffer
FILL = 0xA5
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}
SPECS = fx.map2_palette_specs()


def _spec_index(kind, k):
    (i,) = [i for i, s in enumerate(SPECS) if s["kind"] == kind and s["k"] == k]
    return i


LATTICE32 = _spec_index("lattice", 512)


def _torch_dtype(width):
    import torch
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32}[width]


def _widths_for(k):
    return [w for w in (1, 2, 4) if w == 4 or k - 1 < (1 << (8 * w))]


@pytest.fixture(params=[True, False], ids=["lds", "gather"])
def mappath(gpu, request):
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
    return out


def lowest_labels(colours, pal):
    """The lowest index of each colour in pal (low 24 bits)."""
    p = np.asarray(pal, np.uint32) & np.uint32(0xFFFFFF)
    c = np.asarray(colours, np.uint32) & np.uint32(0xFFFFFF)
    uniq, first = np.unique(p, return_index=True)   # (the first occurrence of each value)
    at = np.searchsorted(uniq, c)
    assert (at < len(uniq)).all() and (uniq[np.minimum(at, len(uniq) - 1)] == c).all(), "a colour outside the palette"
    return first[at].astype(np.uint32)


def _expect(px, pal):
    want = _oracle_map(px, pal)
    lab = lowest_labels(want, pal)
    for a in (want, lab):
        a.setflags(write=False)
    return want, lab


@functools.lru_cache(maxsize=None)
def _map2_case(i):
    """(palette, probe pixels, oracle colours, expected labels) of map2 palette i; computed once, read-only."""
    spec = SPECS[i]
    pal = fx.make_palette(spec)
    px = fx.map_probe_pixels(pal, fx.map2_seed(spec))
    pal.setflags(write=False)
    px.setflags(write=False)
    return (pal, px) + _expect(px, pal)


@functools.lru_cache(maxsize=None)
def _random_case(k, n=None):
    spec = {"k": k, "kind": "random", "seed": 77 + k}
    pal = fx.make_palette(spec)
    px = fx.map_probe_pixels(pal, fx.map2_seed(spec))
    if n is not None:
        px = np.resize(px[max(0, k - 2):], n)
    pal.setflags(write=False)
    px.setflags(write=False)
    return (pal, px) + _expect(px, pal)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


class LabelBuffer:
    """n labels of `width` bytes, `off` bytes past a 256-B aligned address,
    0xA5-filled, with GUARD bytes of 0xA5 on both sides."""

    def __init__(self, n, width, off=0):
        import torch
        assert off % width == 0 and GUARD % 4 == 0
        self.n, self.width, self.off = n, width, off
        self.raw = torch.full((GUARD + off + n * width + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        lo = GUARD + off
        self.t = self.raw[lo:lo + n * width].view(_torch_dtype(width))
        assert self.t.numel() == n and self.t.data_ptr() % 16 == off % 16

    def host(self):
        """The labels, after checking that nothing else was written."""
        import torch
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        lo = GUARD + self.off
        assert (raw[:lo] == FILL).all(), "bytes before the label buffer were written"
        assert (raw[lo + self.n * self.width:] == FILL).all(), "bytes after the label buffer were written"
        return raw[lo:lo + self.n * self.width].view(UNSIGNED[self.width]).copy()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.raw == FILL).all())


def _explain(px, pal, got, want_lab):
    bad = np.flatnonzero(got != want_lab)
    if len(bad) == 0:
        return "labels equal"
    i = int(bad[0])
    return ("K=%d: %d of %d labels differ; first at %d: pixel %08x -> label %d, expected %d (colour %06x)"
            % (len(pal), len(bad), len(px), i, int(px[i]), int(got[i]), int(want_lab[i]),
               int(pal[int(want_lab[i])]) & 0xFFFFFF))


def _check_labels(gpu, px, pal, want, want_lab, width, what="", off_in=0, off_lab=0, t_in=None):
    """One label map against the expectation; returns the labels."""
    import torch
    n = len(px)
    if t_in is None:
        base = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        base[off_in:off_in + n] = _dev(px)
        t_in = base[off_in:off_in + n]
        assert t_in.data_ptr() % 16 == 4 * off_in
    buf = LabelBuffer(n, width, off_lab)
    gpu.map_labels_device(t_in, buf.t, pal)
    got = buf.host()
    assert np.array_equal(got, want_lab), "%s u%d: %s" % (what, 8 * width, _explain(px, pal, got, want_lab))
    assert np.array_equal(np.asarray(pal)[got] & np.uint32(0xFFFFFF), want & np.uint32(0xFFFFFF)), what
    return got


def _check_refused(gpu, px, pal, width):
    buf = LabelBuffer(len(px), width)
    with pytest.raises(gpu.DivQuantError):
        gpu.map_labels_device(_dev(px), buf.t, pal)
    assert buf.untouched()


# ---------------------------------------------------------------------------
MAP_CASES = [("lattice", 512)] + [("cluster", k) for k in (3, 4, 7, 8, 9, 32, 33)] + \
            [("cube", 1000), ("subdivided", 125), ("gray", 2), ("random", 1025), ("random", 16384), ("dups", 2048)]
# (above 1024 entries set_lds_map changes nothing: one run)
MAP_PARAMS = [(kind, k, lds) for kind, k in MAP_CASES for lds in ((True, False) if k <= 1024 else (True,))]


@pytest.mark.parametrize("kind,k,lds", MAP_PARAMS,
                         ids=["%s%d-%s" % (kind, k, "lds" if lds else "gather") for kind, k, lds in MAP_PARAMS])
def test_label_map_probe_pixels(gpu, kind, k, lds):
    """The tie-dense probe pixels of the map2 palettes: lattice (exact ties),
    the inline-count thresholds (3 compact, 7 inline, 32 per-cell cap), one
    cell holding 1000 entries, duplicate entries, K above 1024 -- every legal
    width; an illegal one is refused and writes nothing."""
    pal, px, want, want_lab = _map2_case(_spec_index(kind, k))
    gpu.set_lds_map(lds)
    try:
        for width in (1, 2, 4):
            if width in _widths_for(k):
                _check_labels(gpu, px, pal, want, want_lab, width, "%s%d" % (kind, k))
            else:
                _check_refused(gpu, px, pal, width)
    finally:
        gpu.set_lds_map(True)


def test_lowest_index_rule_is_exercised():
    """The duplicate-entry palette: for some probe pixels the lowest index of
    the answer colour is not its highest, so a table built by "last one wins"
    (or from the sorted order) would fail test_label_map_probe_pixels."""
    pal, px, want, want_lab = _map2_case(_spec_index("dups", 2048))
    p = np.asarray(pal) & np.uint32(0xFFFFFF)
    highest = {int(c): i for i, c in enumerate(p)}
    hi = np.array([highest[int(c) & 0xFFFFFF] for c in want], np.uint32)
    assert (hi != want_lab).any()
    assert (want_lab <= hi).all()


def test_label_255_in_u8(gpu, mappath):
    """A 256-entry palette in u8: the widest u8 label occurs."""
    pal, px, want, want_lab = _random_case(256)
    got = _check_labels(gpu, px, pal, want, want_lab, 1, "random256")
    assert (got == 255).any()
    for width in (2, 4):
        _check_labels(gpu, px, pal, want, want_lab, width, "random256")


def test_k1024_in_u16_and_k1(gpu, mappath):
    """The LDS kernel's largest palette (its 2 KB label table) in u16 and
    u32 -- u8 is refused -- and a palette of one entry in every width."""
    pal, px, want, want_lab = _random_case(1024)
    got = _check_labels(gpu, px, pal, want, want_lab, 2, "random1024")
    assert got.max() == 1023
    _check_labels(gpu, px, pal, want, want_lab, 4, "random1024")
    _check_refused(gpu, px, pal, 1)
    pal, px, want, want_lab = _random_case(1)
    assert not want_lab.any()
    for width in (1, 2, 4):
        _check_labels(gpu, px, pal, want, want_lab, width, "random1")


@functools.lru_cache(maxsize=None)
def _lattice_pixels_case(k):
    """The lattice (step 32) probe pixels -- they straddle its entries and its
    midpoints -- on the lattice itself (k = 512) or on the random palette of k."""
    if k == 512:
        return _map2_case(LATTICE32)
    pal = _random_case(k)[0]
    px = _map2_case(LATTICE32)[1]
    return (pal, px) + _expect(px, pal)


@pytest.mark.parametrize("width,k", [(1, 2), (1, 256), (2, 512), (4, 512), (2, 4096)])
def test_label_map_small_and_ragged(gpu, mappath, width, k):
    """Fewer pixels than one 8-pixel group, one group, a group and a tail,
    ragged sizes of a few workgroups: slices of the lattice probe pixels."""
    pal, px_all, want_all, lab_all = _lattice_pixels_case(k)
    assert len(pal) == k
    for n in (1, 5, 7, 8, 9, 15, 8197, 16389):
        off = 500 + n % 7
        s = slice(off, off + n)
        _check_labels(gpu, px_all[s], pal, want_all[s], lab_all[s], width, "n=%d" % n)


def test_label_map_many_iterations(gpu):
    """map_lds_kernel, u8, 3000005 pixels: more groups per workgroup than its
    1024 lanes -- a second, partial iteration of the prefetch pipeline, then
    the tail.  A block of 8 x 7501 probe pixels of a 256-entry palette,
    repeated."""
    import torch
    pal, px, _, _ = _random_case(256)
    blk = np.resize(px, 8 * 7501)
    ref, ref_lab = _expect(blk, pal)
    n = 3000005
    reps = (n + len(blk) - 1) // len(blk)
    t_in = _dev(blk).repeat(reps)[:n].contiguous()
    buf = LabelBuffer(n, 1)
    gpu.set_lds_map(True)
    gpu.map_labels_device(t_in, buf.t, pal)
    torch.cuda.synchronize()
    t_ref = torch.from_numpy(ref_lab.astype(np.uint8)).to("cuda:0")
    full = n // len(blk)
    head = buf.t[:full * len(blk)].view(full, -1)
    if not bool((head == t_ref).all()) or not torch.equal(buf.t[full * len(blk):], t_ref[:n - full * len(blk)]):
        pytest.fail(_explain(np.resize(blk, n), pal, buf.host(), np.resize(ref_lab, n)))
    buf.host()   # (the guards)


@pytest.mark.parametrize("k", [16, 2000])
@pytest.mark.parametrize("n", [5, 70001])
def test_label_map_misaligned(gpu, mappath, n, k):
    """Input 4 B off 16-B alignment, a u8 label pointer 1 and 3 bytes off, a
    u16 one 2 bytes off (naturally aligned, staged), then an aligned call on
    the same engine; the guards show that only the n labels are written."""
    pal, px, want, want_lab = _random_case(k, n)
    cases = [(1, 2, 0), (0, 2, 2), (1, 2, 2), (0, 4, 4)]
    if k <= 256:
        cases += [(1, 1, 0), (0, 1, 1), (0, 1, 3), (1, 1, 3)]
    for off_in, width, off_lab in cases:
        _check_labels(gpu, px, pal, want, want_lab, width, "offsets (%d, %d)" % (off_in, off_lab),
                      off_in=off_in, off_lab=off_lab)
    for width in _widths_for(k):
        _check_labels(gpu, px, pal, want, want_lab, width, "aligned after staged")


def test_label_and_colour_call_sequence(gpu):
    """One engine: label u8 K=256, colour K=16384, label u16 K=1024, the colour
    map of that same palette, label u32 K=3.  A label task's cell table holds
    labels where a colour task's holds colours: neither may leak into the
    next call on the same palette."""
    import torch

    def colour(case, what):
        pal, px, want, _ = case
        t_out = torch.full((len(px),), int(np.uint32(0xA5A5A5A5).view(np.int32)), dtype=torch.int32, device="cuda:0")
        gpu.map_device(_dev(px), t_out, pal)
        torch.cuda.synchronize()
        got = t_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), "%s: %d colours differ" % (what, int((got != want).sum()))

    def labels(case, width, what):
        pal, px, want, want_lab = case
        _check_labels(gpu, px, pal, want, want_lab, width, what)

    gpu.set_lds_map(True)
    k1024 = _random_case(1024)
    labels(_random_case(256), 1, "step 0")
    colour(_map2_case(_spec_index("random", 16384)), "step 1")
    labels(k1024, 2, "step 2")
    colour(k1024, "step 3")
    labels(k1024, 4, "step 4 (labels again)")
    labels(_map2_case(_spec_index("cluster", 3)), 4, "step 5")


# ---------------------------------------------------------------------------
# quant: labels in place of colours
def _quant_labels_dev(gpu, frames, k, width, uniq=1):
    """quant_labels_batch_device over host frames; returns ([labels], [ct], empty)."""
    t_ins = [_dev(px) for px in frames]
    bufs = [LabelBuffer(len(px), width) for px in frames]
    cts, empty = gpu.quant_labels_batch_device(t_ins, [b.t for b in bufs], k, all_pixels_unique=uniq)
    return [b.host() for b in bufs], cts, empty


def _hash(a):
    return "%016x" % fx.fnv(a)


@pytest.mark.parametrize("width", [1, 4])
def test_quant_labels_batch_cases(gpu, width):
    """Three cases.json inputs of different n in one call: the fixture's
    colortables, labels that reproduce its mapped output, and the empty
    count of quant_batch_device."""
    import torch
    cases = fx.load_json("cases.json")
    pick = [c for c in cases if c["spec"]["k"] == 16 and c["spec"]["kind"] == "uniform"
            and c["spec"]["n"] in (257, 1000, 65536)]
    assert sorted(c["spec"]["n"] for c in pick) == [257, 1000, 65536]
    frames = [fx.make_case(c["spec"]) for c in pick]
    labels, cts, empty = _quant_labels_dev(gpu, frames, 16, width)
    for c, lab, ct in zip(pick, labels, cts):
        assert [int(v) for v in ct] == c["ct"], c["spec"]
        assert lab.max() < len(ct)
        assert _hash(ct[lab]) == c["out_fnv"], c["spec"]
    t_ins = [_dev(px) for px in frames]
    cts2, empty2 = gpu.quant_batch_device(t_ins, [torch.empty_like(t) for t in t_ins], 16)
    assert empty == empty2
    assert all(np.array_equal(a, b) for a, b in zip(cts, cts2))


@pytest.mark.parametrize("name", ["batman", "cookie"])
@pytest.mark.parametrize("k", [4, 16, 125, 256])
def test_quant_labels_sample_images(gpu, name, k):
    """The reference's sample images, both allPixelsUnique values, u8: the
    labels index the reference build's colortable and reproduce its output."""
    fix = fx.load_json("png.json")[name]
    px, w, h = fx.load_png_u32(fx.os.path.join(fx.GOLDEN, "png", name + ".png"))
    for uniq, key in ((1, "k%d" % k), (0, "k%d_weighted" % k)):
        (lab,), (ct,), _ = _quant_labels_dev(gpu, [px], k, 1, uniq=uniq)
        assert [int(v) for v in ct] == fix[key]["ct"], key
        assert _hash(ct[lab]) == fix[key]["out_fnv"], key


@pytest.mark.parametrize("wsmall", [True, False], ids=["wsmall", "rounds"])
def test_quant_labels_weighted_regions(gpu, wsmall):
    """Eight weighted2.json cases at K = 4 (the app's per-region call), u8,
    through the one-launch kernel (cluster + dedup there, labels by the map
    kernels) and through the weighted rounds."""
    cases = [c for c in fx.load_json("weighted2.json") if c["spec"]["k"] == 4]
    pick = [c for c in cases if not c["spec"]["kind"].startswith("crop_")][:4] + \
           [c for c in cases if c["spec"]["kind"].startswith("crop_")][:4]
    assert len(pick) == 8
    gpu.set_wsmall(wsmall)
    try:
        for c in pick:
            px = fx.make_weighted_case(c["spec"])
            (lab,), (ct,), _ = _quant_labels_dev(gpu, [px], 4, 1, uniq=0)
            assert [int(v) for v in ct] == c["ct"], c["spec"]
            assert _hash(ct[lab]) == c["out_fnv"], c["spec"]
    finally:
        gpu.set_wsmall(True)


def test_quant_labels_above_256(gpu):
    """K = 300 in u16 against quant_device of the same build; u8 cannot hold
    index 299: refused before any work, the buffer left as it was."""
    import torch
    px = gpu.synth_frame(256 * 256, 0)
    t_in = _dev(px)
    t_out = torch.empty_like(t_in)
    ct_ref, empty_ref = gpu.quant_device(t_in, t_out, 300)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy().view(np.uint32)
    (lab,), (ct,), empty = _quant_labels_dev(gpu, [px], 300, 2)
    assert np.array_equal(ct, ct_ref) and empty == empty_ref
    assert lab.max() > 255
    assert np.array_equal(ct[lab], out)
    buf = LabelBuffer(len(px), 1)
    with pytest.raises(gpu.DivQuantError):
        gpu.quant_labels_batch_device([t_in], [buf.t], 300)
    assert buf.untouched()


def test_quant_labels_host_pointers(gpu):
    """quant_labels on host arrays: a known-answer input and a cases.json
    case, default width (u8) and u32."""
    px, k = fx.kat_inputs()["testQuant_4x4_N16"]
    fix = fx.load_json("kats.json")["testQuant_4x4_N16"]
    for dtype in (None, np.uint32):
        lab, ct = gpu.quant_labels(px, k, 1, dtype=dtype)
        assert lab.dtype == (np.uint8 if dtype is None else dtype)
        assert [int(v) for v in ct] == fx.KAT_EXPECTED["testQuant_4x4_N16"]
        assert [int(v) for v in ct[lab]] == fix["out"]
    (c,) = [c for c in fx.load_json("cases.json")
            if c["spec"]["n"] == 4099 and c["spec"]["k"] == 300 and c["spec"]["kind"] == "clustered"]
    lab, ct = gpu.quant_labels(fx.make_case(c["spec"]), 300)
    assert lab.dtype == np.uint16
    assert [int(v) for v in ct] == c["ct"]
    assert _hash(ct[lab]) == c["out_fnv"]
