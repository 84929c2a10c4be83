"""The device head trim on the heads of tests/_trim_cases.py (tests/test_trim_cases.py holds them to the
reference on the CPU and shows which wrong scans they tell apart).  The C ABI takes one pgn_trim_params per
call, so the cases are grouped by parameters: one PGNanoCodec.segment_reads call per group, the reads packed
back to back behind one leading sample, an odd-length plain read first so that the starts fall on odd and even
2-byte boundaries.  Per read trim, head_m2, head_mad4, status, first_segment, nsegments and the bits of
threshold, then the statistics, the segment table and every row at L 64, V 16, against ref_batch
(tests/test_segment_api.py): the tolerance is zero, for the NaN threshold of 0 * inf too (the device and the
reference's x86 host both make 0xffc00000 of it).

The heads above 1,024 samples run under the context's own split settings (the workgroup selection), under
set_select_split(1024, 1024, 1024) (the head is selected in parts) and with max_split_reads = 0: the same bytes
everywhere.  select_split_counts() describes a call's last selection -- the trimmed reads -- so that the heads
split is asserted on the inputs, max_samples and H above split_min_samples, and the counters are held to the
trimmed lengths (they are all 0 when a call ran with the split off).

One call of more reads than the trim and table kernels' grids cover in one round (min((nreads + 3) / 4,
64 * CUs) workgroups of four waves), against a reference vectorised in NumPy, and the refusal of non-finite
parameters with canary-filled outputs.
"""
import ctypes as C
import time

import numpy as np
import pytest

import _oracle as O
import _trim_cases as T
from test_gpu_segments import BITS, NP_OF, SENTINEL, dev, sentinel_out, tdtype
from test_gpu_select_split import expected_counts
from test_norm_api import QUANTILE, assert_stats_equal, f32_bits
from test_segment_api import ref_batch, ref_segments

pytestmark = pytest.mark.gpu

L, V = 64, 16
f32 = np.float32
SMALL = dict(split_min_samples=1024, part_samples=1024, max_split_reads=1024)
GROUPS = T.groups()
IDS = [f"{g[1][0].name}+{len(g[1]) - 1}" for g in GROUPS]
_REF = {}


class Group:
    """One parameter set's cases behind a plain read of odd length, and their reference (computed once)."""

    def __init__(self, i):
        self.prm, self.cases = GROUPS[i]
        self.names = ["plain"] + [c.name for c in self.cases]
        self.reads = [O.synth_read(4000 + i, 301)] + [c.x for c in self.cases]
        self.counts = np.array([r.size for r in self.reads], np.int64)
        self.offsets = 1 + np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)
        self.flat = np.concatenate([np.array([12345], np.int16)] + self.reads)
        assert (self.offsets % 2 == 1).any() and (self.offsets % 2 == 0).any()
        with np.errstate(all="ignore"):
            self.want = ref_batch(self.reads, L, V, self.prm, QUANTILE)
        for c, w in zip(self.cases, self.want["reads"][1:]):  # the reference gives what the case claims
            assert (w["trim"], w["head_m2"], w["head_mad4"]) == (c.trim, c.m2, c.mad4), c.name


def group(i):
    if i not in _REF:
        _REF[i] = Group(i)
    return _REF[i]


def run(codec, g, dtype):
    """One call into a sentinel-filled output: (res, the bytes of everything it wrote)."""
    cap = g.want["total"] + 2
    buf, out = sentinel_out(cap, L, dtype)
    res = codec.segment_reads(dev(g.flat), dev(g.offsets), g.counts, length=L, overlap=V, trim=g.prm, dtype=tdtype(dtype),
                              out=out, **QUANTILE)
    host = buf.cpu().numpy().view(BITS[dtype])
    assert (host[g.want["total"] * L:] == SENTINEL[dtype]).all(), "rows at or above total were written"
    k = g.want["total"]
    return res, (res.reads.numpy().tobytes(), res.segments.numpy()[:k].tobytes(), res.stats.numpy().tobytes(),
                 host[:k * L].tobytes())


def compare(res, g, dtype, what):
    want = g.want
    wrong = []
    if int(res.total.item()) != want["total"]:
        wrong.append(f"total {int(res.total.item())}, want {want['total']}")
    got = res.reads.numpy()
    for r, w in enumerate(want["reads"]):
        for k in ("trim", "head_m2", "head_mad4", "status", "first_segment", "nsegments"):
            if int(got[r][k]) != int(w[k]):
                wrong.append(f"{g.names[r]}: {k} = {int(got[r][k])}, want {int(w[k])}")
        if f32_bits(got[r]["threshold"]) != f32_bits(w["threshold"]):
            wrong.append(f"{g.names[r]}: threshold = {got[r]['threshold']!r} ({f32_bits(got[r]['threshold']):#010x}), want "
                         f"{w['threshold']!r} ({f32_bits(w['threshold']):#010x})")
    assert not wrong, f"{what}: " + "; ".join(wrong[:12]) + (f" (+{len(wrong) - 12} more)" if len(wrong) > 12 else "")
    stats = res.stats.numpy()
    for r, w in enumerate(want["stats"]):
        assert_stats_equal(stats[r], w, f"{what}: {g.names[r]}")
    k = want["total"]
    segs = res.segments.numpy()[:k]
    assert np.array_equal(np.stack([segs["read"], segs["start"], segs["valid"]], 1).astype(np.int64), want["segments"]), what
    with np.errstate(over="ignore"):
        rows = want["rows32"].astype(NP_OF[dtype])
    out = res.out.cpu().numpy()[:k]
    diff = np.argwhere(out.view(BITS[dtype]) != rows.view(BITS[dtype]))
    assert not len(diff), f"{what}: {len(diff)} values differ, first at row {diff[0][0]} column {diff[0][1]}"


def test_the_groups_hold_every_case():
    names = [c.name for _, cases in GROUPS for c in cases]
    assert sorted(names) == sorted(c.name for c in T.catalogue()) and len(GROUPS) >= 20
    assert any(c.outcome == "no_window" and c.x.size < c.prm["min_trim"] for c in T.catalogue())  # an empty trimmed read


@pytest.mark.parametrize("i", range(len(GROUPS)), ids=IDS)
def test_cases_float16(codec, i):
    g = group(i)
    res, _ = run(codec, g, "float16")
    compare(res, g, "float16", f"group {IDS[i]}")
    for c, w in zip(g.cases, g.want["reads"][1:]):
        if c.x.size <= c.trim:  # n <= min_trim: the trimmed read is empty, no segments, status 0
            assert w["nsegments"] == 0 and w["status"] == 0


@pytest.mark.parametrize("i", [i for i, g in enumerate(GROUPS) if len(g[1]) >= 6], ids=lambda i: IDS[i])
def test_cases_float32(codec, i):
    g = group(i)
    res, _ = run(codec, g, "float32")
    compare(res, g, "float32", f"group {IDS[i]} float32")


LARGE = [i for i, g in enumerate(GROUPS) if any(c.cls == "workgroup" for c in g[1])]


@pytest.mark.parametrize("i", LARGE, ids=lambda i: IDS[i])
def test_large_heads_under_every_selection(codec, i):
    g = group(i)
    big = [c for c in g.cases if c.cls == "workgroup"]
    assert g.prm["max_samples"] > SMALL["split_min_samples"] and all(c.H > SMALL["split_min_samples"] for c in big)
    before = codec.select_split
    assert all(c.H <= before[0] for c in big) or before[2] == 0, "the context's own settings already split these heads"
    try:
        res, own = run(codec, g, "float16")
        compare(res, g, "float16", f"group {IDS[i]}, the context's settings")
        codec.set_select_split(**SMALL)
        res, parts = run(codec, g, "float16")
        compare(res, g, "float16", f"group {IDS[i]}, heads in parts")
        # the counters are those of the call's last selection, the trimmed reads: it ran with the split on
        trimmed = [int(n) - int(r["trim"]) for n, r in zip(g.counts, g.want["reads"])]
        got = codec.select_split_counts()
        assert got == expected_counts(trimmed) and got["short"] + got["whole"] + got["split"] == len(trimmed), got
        codec.set_select_split(max_split_reads=0)
        res, off = run(codec, g, "float16")
        assert codec.select_split_counts()["split"] == 0
    finally:
        codec.set_select_split(*before)
    assert codec.select_split == before
    for a, b, c in zip(own, parts, off):
        assert a == b == c, "the split changes the bytes"


def test_both_head_size_classes_are_run():
    assert len(LARGE) >= 4
    cls = {c.cls for _, cases in GROUPS for c in cases}
    assert cls == {"none", "wave", "workgroup"}


# ---- more reads than one round of the grid -------------------------------------------------------------------
MANY = dict(max_samples=48, window=4, min_elements=1, min_trim=2, mad_mult=1.0, threshold_mads=1.5)
ML, MV = 32, 8


def many_reads(R, n=64):
    """[R, n] int16: a narrow band with one burst of raised samples per read, anywhere in the head."""
    rng = np.random.default_rng(1164)
    X = rng.integers(90, 111, (R, n)).astype(np.int16)
    start, length = rng.integers(0, 44, R), rng.integers(0, 14, R)
    col = np.arange(n)[None, :]
    X[(col >= start[:, None]) & (col < (start + length)[:, None])] = 200
    return X


def vector_reference(X, status):
    """ref_batch of equal-length reads, vectorised: np.sort along axis 1 and the rule's float32 steps."""
    R, n = X.shape
    T_ = MANY
    H, window, min_trim = min(n, T_["max_samples"]), T_["window"], T_["min_trim"]
    head = X[:, :H].astype(np.int64)
    s = np.sort(head, axis=1)
    m2 = s[:, (H - 1) // 2] + s[:, H // 2]
    t = np.sort(np.abs(2 * head - m2[:, None]), axis=1)
    mad4 = t[:, (H - 1) // 2] + t[:, H // 2]
    thr = f32(0.5) * m2.astype(f32) + f32(T_["threshold_mads"]) * (f32(T_["mad_mult"]) * (f32(0.25) * mad4.astype(f32)))
    assert thr.dtype == np.float32
    above = X[:, :H].astype(f32) > thr[:, None]
    W = (H - min_trim) // window
    win = above[:, min_trim:min_trim + W * window].reshape(R, W, window)
    seen = np.maximum.accumulate(win.sum(axis=2) > T_["min_elements"], axis=1)
    stop = seen & ~win[:, :, -1]
    e = min_trim + (stop.argmax(axis=1) + 1) * window
    trim = np.where(stop.any(axis=1) & (e < H), e, min_trim)
    bad = status != 0
    for a in (trim, m2, mad4, thr):
        a[bad] = 0
    nseg = np.zeros(R, np.int64)
    q = dict(a=np.zeros(R, np.int64), b=np.zeros(R, np.int64), centre=np.zeros(R, f32), spread=np.ones(R, f32))
    plans, rows = {}, {}
    for tr in np.unique(trim[~bad]):
        idx = np.flatnonzero((trim == tr) & ~bad)
        Y = X[idx, tr:]
        m = n - int(tr)
        ys = np.sort(Y.astype(np.int64), axis=1)
        a = ys[:, int(np.floor(np.float64(QUANTILE["p"][0]) * np.float64(m - 1)))]
        b = ys[:, int(np.floor(np.float64(QUANTILE["p"][1]) * np.float64(m - 1)))]
        centre = f32(QUANTILE["centre_mult"]) * (a + b).astype(f32)
        spread = np.maximum(f32(QUANTILE["spread_mult"]) * (b - a).astype(f32), f32(QUANTILE["spread_floor"]))
        z = (Y.astype(f32) + (-centre)[:, None]) * (f32(1.0) / spread)[:, None]
        assert z.dtype == np.float32
        plan = ref_segments(m, ML, MV)
        block = np.zeros((idx.size, len(plan), ML), f32)
        for j, (st, valid) in enumerate(plan):
            block[:, j, :valid] = z[:, st:st + valid]
        plans[int(tr)], rows[int(tr)] = plan, (idx, block)
        nseg[idx] = len(plan)
        q["a"][idx], q["b"][idx], q["centre"][idx], q["spread"][idx] = a, b, centre, spread
    first = np.concatenate([[0], np.cumsum(nseg)[:-1]])
    total = int(nseg.sum())
    rows32 = np.zeros((total, ML), f32)
    segs = np.zeros((total, 3), np.int64)
    for tr, (idx, block) in rows.items():
        for j, (st, valid) in enumerate(plans[tr]):
            rows32[first[idx] + j] = block[:, j]
            segs[first[idx] + j] = np.stack([idx, np.full(idx.size, tr + st), np.full(idx.size, valid)], 1)
    return dict(trim=trim, m2=m2, mad4=mad4, thr=thr, nseg=nseg, first=first, total=total, rows32=rows32, segs=segs, q=q)


def test_more_reads_than_one_round_of_the_grid(codec):
    """4 * 64 * CUs + 37 reads of 64 samples: the trim and the table kernels' grids take 4 * 64 * CUs reads per
    round, so the last 37 are a second round, and the segment scan takes 1,024 reads per step.  Every
    eleventh read carries an input status."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = 4 * 64 * cus + 37
    assert (R + 3) // 4 > 64 * cus and R > 20 * 1024
    t0 = time.perf_counter()
    X = many_reads(R)
    status = np.where(np.arange(R) % 11 == 10, 6, 0).astype(np.int32)
    want = vector_reference(X, status)
    # the vectorised reference is ref_batch on the reads it can be run on in a moment
    k = 60
    small = ref_batch(list(X[:k]), ML, MV, MANY, QUANTILE, status_in=status[:k])
    assert [r["trim"] for r in small["reads"]] == want["trim"][:k].tolist()
    assert [r["first_segment"] for r in small["reads"]] == want["first"][:k].tolist()
    assert np.array_equal(small["rows32"].view(np.uint32), want["rows32"][:small["total"]].view(np.uint32))
    assert np.array_equal(small["segments"], want["segs"][:small["total"]])
    assert len(set(want["trim"][status == 0].tolist())) >= 6, "the bursts should end in many windows"
    t1 = time.perf_counter()
    flat = np.concatenate([np.array([12345], np.int16), X.reshape(-1)])
    offsets = 1 + 64 * np.arange(R, dtype=np.int64)
    counts = np.full(R, 64, np.int64)
    cap = want["total"] + 2
    buf, out = sentinel_out(cap, ML, "float16")
    res = codec.segment_reads(dev(flat), dev(offsets), counts, length=ML, overlap=MV, trim=MANY, dtype=torch.float16,
                              read_status=dev(status), out=out, **QUANTILE)
    assert int(res.total.item()) == want["total"]
    t2 = time.perf_counter()
    got = res.reads.numpy()
    good = status == 0
    for k, w in (("trim", want["trim"]), ("head_m2", want["m2"]), ("head_mad4", want["mad4"]), ("nsegments", want["nseg"]),
                 ("first_segment", want["first"]), ("status", status)):
        at = np.flatnonzero(got[k].astype(np.int64) != w)
        assert not at.size, f"{k}: {at.size} reads differ, first read {at[0]}: {got[k][at[0]]}, want {w[at[0]]}"
    assert np.array_equal(got["threshold"].view(np.uint32), want["thr"].view(np.uint32))
    st = res.stats.numpy()
    assert np.array_equal(st["n"][good].astype(np.int64), 64 - want["trim"][good]) and (st["status"][good] == 0).all()
    assert np.array_equal(st["q_lo"][good], want["q"]["a"][good]) and np.array_equal(st["q_hi"][good], want["q"]["b"][good])
    for k in ("centre", "spread"):
        assert np.array_equal(st[k][good].view(np.uint32), want["q"][k][good].view(np.uint32)), k
    segs = res.segments.numpy()[:want["total"]]
    assert np.array_equal(np.stack([segs["read"], segs["start"], segs["valid"]], 1).astype(np.int64), want["segs"])
    host = buf.cpu().numpy().view(np.uint16)
    rows = want["rows32"].astype(np.float16).view(np.uint16)
    diff = np.argwhere(host[:want["total"] * ML].reshape(-1, ML) != rows)
    assert not len(diff), f"{len(diff)} values differ, first at row {diff[0][0]} column {diff[0][1]}"
    assert (host[want["total"] * ML:] == SENTINEL["float16"]).all()
    t3 = time.perf_counter()
    print(f"{R} reads ({cus} CUs), {want['total']} rows: data and reference {t1 - t0:.2f} s, call {t2 - t1:.2f} s, "
          f"compare {t3 - t2:.2f} s")
    assert t3 - t0 < 30.0, "the many-reads call has become slow"


# ---- refusal ---------------------------------------------------------------------------------------------
def test_nonfinite_parameters_are_refused(codec):
    """mad_mult or threshold_mads inf or NaN: PGN_ERR_INVALID_ARG, and no output is touched."""
    import torch

    from rawnanoporesignalcompression_amd import _native, norm_params, segment_params, trim_params

    g = group(0)
    d_flat, d_off, d_cnt = dev(g.flat), dev(g.offsets), dev(g.counts)
    n, cap = len(g.reads), g.want["total"] + 2
    canary = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    outs = [canary(cap * L * 2), canary(cap * C.sizeof(_native.Segment)), canary(n * C.sizeof(_native.ReadSegments)),
            canary(n * C.sizeof(_native.ReadStats)), canary(8)]
    prm, seg = norm_params(**QUANTILE), segment_params(L, V)
    inf, nan = float("inf"), float("nan")
    bad = [dict(mad_mult=inf), dict(mad_mult=-inf), dict(mad_mult=nan), dict(threshold_mads=inf),
           dict(threshold_mads=-inf), dict(threshold_mads=nan)]
    for kw in bad:
        t = trim_params(**dict(g.prm, **kw))
        rc = codec._lib.pgn_segment_reads_device(codec._h, n, d_flat.data_ptr(), d_off.data_ptr(), d_cnt.data_ptr(), None,
                                                 C.byref(t), C.byref(prm), C.byref(seg), outs[0].data_ptr(),
                                                 _native.PGN_OUT_F16, cap, outs[1].data_ptr(), outs[2].data_ptr(),
                                                 outs[3].data_ptr(), outs[4].data_ptr(), None)
        assert rc == _native.PGN_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == 0xA5).all(), "a refused call wrote to its outputs"
    # the largest finite mad_mult is accepted: the non-finite threshold cases run with it
    assert any(c.prm["mad_mult"] == 3e38 for c in T.catalogue())
