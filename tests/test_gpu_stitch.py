"""Model output back to reads on the GPU (PGNanoCodec.stitch_plan / stitch over pgn_stitch_plan_device /
pgn_stitch_rows_device), bit for bit against the numpy rule (stitch_plan_signal, which tests/test_stitch_api.py
holds to the header's text) applied to the tables the segment call left: an index computation and a byte copy,
so the tolerance is zero.  Shapes are small on purpose; what they reach is named at each test.
"""
import os

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

CONFIGS = [(8, 0, 8), (8, 4, 4), (40, 8, 4), (40, 7, 4), (48, 12, 6)]  # (L, V, s): T = 1; S == s; regular; odd V; s = 6
FRAME_BYTES = [1, 2, 6, 16, 18, 48]
TRIM = dict(max_samples=100, window=7, min_elements=1, min_trim=3, mad_mult=1.0, threshold_mads=1.5)
LONG_SEGMENTS = 2100
BAD_STATUS = 6
CANARY = 0xA5


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def ref_tables(reads, segs, capacity, L, V, s):
    """(plan, read_frames) the plan call must leave for these downloaded tables: pgn_stitch_segment records
    for rows [0, min(total, capacity)), and the nreads + 1 frame offsets."""
    from rawnanoporesignalcompression_amd import StitchTable, stitch_plan_signal

    n = len(reads)
    total = int(reads["first_segment"][-1]) + int(reads["nsegments"][-1]) if n else 0
    nrows = min(total, capacity)
    plan = np.zeros(nrows, StitchTable.DTYPE)
    frames = np.zeros(n + 1, np.int64)
    pos = 0
    for r in range(n):
        frames[r] = pos
        first, k = int(reads["first_segment"][r]), int(reads["nsegments"][r])
        if reads["status"][r] == 0 and k >= 1 and first + k <= capacity:
            rows = segs[first:first + k]
            fc = stitch_plan_signal(np.stack([rows["start"], rows["valid"]], 1), L, V, s)
            plan["first"][first:first + k] = fc[:, 0]
            plan["count"][first:first + k] = fc[:, 1]
            plan["dst_frame"][first:first + k] = pos + np.cumsum(fc[:, 1]) - fc[:, 1]
            pos += int(fc[:, 1].sum())
        else:
            plan["dst_frame"][first:min(first + k, nrows)] = pos
    frames[n] = pos
    return plan, frames


def check_plan(got, want_plan, want_frames, what):
    g = got.segments.numpy()[:len(want_plan)]
    for col in ("first", "count", "dst_frame"):
        if not np.array_equal(g[col], want_plan[col]):
            bad = np.flatnonzero(g[col] != want_plan[col])
            raise AssertionError(f"{what}: {col} differs in {bad.size} of {len(g)} rows, first at row {bad[0]}: "
                                 f"got {g[col][bad[0]]}, want {want_plan[col][bad[0]]}")
    assert np.array_equal(got.read_frames.cpu().numpy(), want_frames), what
    # the named columns are views of the same bytes
    assert np.array_equal(got.segments.count.cpu().numpy()[:len(g)], g["count"].astype(np.int32))
    assert np.array_equal(got.segments.dst_frame.cpu().numpy()[:len(g)], g["dst_frame"].astype(np.int64))


class Case:
    """One batch cut with (L, V) and its plan for stride s, device and reference: reads of the lengths at which
    the segment count or the last row's alignment changes, a couple of hundred random ones, one read with a bad
    input status and one of more than LONG_SEGMENTS segments (its prefix crosses waves and workgroups)."""

    def __init__(self, codec, L, V, s, trim):
        S = L - V
        rng = np.random.default_rng(1000 * L + 10 * V + s)
        lengths = [0, 1, s - 1, s, L - 1, L, L + 1, L + S - 1, L + S, L + S + 1]
        lengths += rng.integers(0, 8 * L, 200).tolist() + [L + (LONG_SEGMENTS + 30) * S + 3] + rng.integers(0, 3 * L, 20).tolist()
        if trim:  # room for the head the trim takes, so the trimmed lengths still reach the edges
            lengths = [n + int(rng.integers(0, 12)) for n in lengths]
        reads = [O.synth_read(3000 + i, int(n)) for i, n in enumerate(lengths)]
        counts = np.array([r.size for r in reads], np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        status = np.zeros(len(reads), np.int32)
        self.bad = 40
        status[self.bad] = BAD_STATUS
        self.L, self.V, self.s, self.T = L, V, s, L // s
        self.segmented = codec.segment_reads(dev(np.concatenate(reads)), offsets, counts, length=L, overlap=V,
                                             trim=TRIM if trim else None, read_status=dev(status), mode="medmad")
        self.reads, self.segs = self.segmented.reads.numpy(), self.segmented.segments.numpy()
        self.total = int(self.segmented.total.item())
        assert self.total <= len(self.segs) and (self.reads["status"] == status).all()
        self.plan = codec.stitch_plan(self.segmented, L, V, s)
        self.want_plan, self.want_frames = ref_tables(self.reads, self.segs, len(self.segs), L, V, s)
        self.frames = int(self.want_frames[-1])


@pytest.fixture(scope="module")
def cases(codec):
    made = {}

    def get(cfg, trim=True):
        if (cfg, trim) not in made:
            made[cfg, trim] = Case(codec, *cfg, trim)
        return made[cfg, trim]

    return get


@pytest.mark.parametrize("trim", [False, True], ids=["untrimmed", "trimmed"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=str)
def test_plan(cases, cfg, trim):
    """first, count, dst_frame of every row and read_frames.  Untrimmed, the reads have exactly the lengths
    0, 1, s-1, s, L-1, L, L+1, L+S-1, L+S, L+S+1; trimmed, start_0 != 0; one read carries a bad status and gives
    no frames; one has more than 2,100 segments."""
    c = cases(cfg, trim)
    check_plan(c.plan, c.want_plan, c.want_frames, f"{cfg} trim={trim}")
    assert c.reads["nsegments"].max() >= LONG_SEGMENTS and c.total > 2 * 1024
    assert c.want_frames[c.bad] == c.want_frames[c.bad + 1] and c.reads["status"][c.bad] == BAD_STATUS
    assert len(c.plan.read_frames) == len(c.reads) + 1 and c.frames > 0
    first = c.segs["start"][c.reads["first_segment"][c.reads["nsegments"] > 0]]
    assert (first != 0).any() if trim else (first == 0).all()


def test_plan_many_tiny_reads(codec):
    """3,000 reads of a few segments each: the scan crosses the count kernel's workgroups read by read."""
    L, V, s = 8, 4, 4
    rng = np.random.default_rng(77)
    counts = rng.integers(0, 3 * L, 3000).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    flat = O.synth_read(88, int(counts.sum()))
    seg = codec.segment_reads(dev(flat), offsets, counts, length=L, overlap=V, mode="medmad")
    reads, segs = seg.reads.numpy(), seg.segments.numpy()
    assert int(seg.total.item()) > 3 * 1024
    plan = codec.stitch_plan(seg, L, V, s)
    check_plan(plan, *ref_tables(reads, segs, len(segs), L, V, s), "tiny reads")


def test_plan_capacity_cuts_a_read(codec):
    """A segment capacity in the middle of a read: the segment call gives that read and every later one with
    segments PGN_ERR_DST_TOO_SMALL, and they yield no frames.  Then a plan capacity below the table's own, with
    the table rows from it on overwritten: they are never read, and the read the capacity cuts yields no frames
    although its status is PGN_OK."""
    import torch

    L, V, s = 40, 7, 4
    counts = np.array([100, 333, 40, 0, 500, 90], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    flat = dev(O.synth_read(99, int(counts.sum())))
    full = codec.segment_reads(flat, offsets, counts, length=L, overlap=V, mode="medmad")
    nseg = full.reads.numpy()["nsegments"].astype(np.int64)
    cut = int(nseg[:4].sum() + 3)  # three rows into read 4
    assert nseg[4] > 4
    short = codec.segment_reads(flat, offsets, counts, length=L, overlap=V, mode="medmad", capacity=cut)
    reads, segs = short.reads.numpy(), short.segments.numpy()
    assert reads["status"].tolist() == [0, 0, 0, 0, 1, 1] and len(segs) == cut
    want_plan, want_frames = ref_tables(reads, segs, cut, L, V, s)
    assert want_frames[4] == want_frames[6] and (want_plan["count"][-3:] == 0).all() and want_frames[4] > 0
    check_plan(codec.stitch_plan(short, L, V, s), want_plan, want_frames, "segment capacity")

    reads, segs = full.reads.numpy(), full.segments.numpy()
    want_plan, want_frames = ref_tables(reads, segs, cut, L, V, s)
    assert (reads["status"] == 0).all() and want_frames[4] == want_frames[6]
    full.segments.raw[cut:] = 0xFF
    got = codec.stitch_plan(full, L, V, s, capacity=cut)
    assert len(got.segments) == cut
    check_plan(got, want_plan, want_frames, "plan capacity")
    torch.cuda.synchronize()


def test_plan_without_reads(codec):
    empty = codec.segment_reads(dev(np.zeros(4, np.int16)), [], [], length=8, overlap=4)
    plan = codec.stitch_plan(empty, 8, 4, 4)
    assert plan.read_frames.cpu().tolist() == [0] and len(plan.segments) == 0


# ---- the rows --------------------------------------------------------------------------------------
def offset_buffer(nbytes, fill=None, lead=2):
    """A uint8 device buffer and the offset in it of `nbytes` that start `lead` bytes behind a 16-byte
    boundary, with at least 16 bytes in front and behind."""
    import torch

    buf = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    if fill is not None:
        buf.fill_(fill)
    off = (-buf.data_ptr()) % 16 + 16 + lead
    return buf, off


def device_rows(host, time_major):
    """host [N, T, fb] uint8 -> a device tensor of that shape or [T, N, fb], 2 bytes off a 16-byte boundary."""
    import torch

    laid = np.ascontiguousarray(host.transpose(1, 0, 2)) if time_major else host
    buf, off = offset_buffer(laid.size)
    view = buf[off:off + laid.size].view(*laid.shape)
    view.copy_(torch.from_numpy(laid))
    assert view.data_ptr() % 16 == 2
    return view


def ref_gather(canvas, plan, rows, g0, base):
    """Write the kept frames of plan rows [g0, g0 + N) into canvas [cap, fb] (rows: [N, T, fb]), as the rows call
    defines: frame f of row g to canvas[dst_frame + (f - first) - base], where that lies in the canvas."""
    p = plan[g0:g0 + rows.shape[0]]
    cnt = p["count"].astype(np.int64)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    row = np.repeat(np.arange(len(p)), cnt)
    f = np.repeat(p["first"].astype(np.int64), cnt) + within
    d = np.repeat(p["dst_frame"].astype(np.int64), cnt) + within - base
    ok = (d >= 0) & (d < canvas.shape[0])
    canvas[d[ok]] = rows[row[ok], f[ok]]
    return int(ok.sum())


def run_rows(codec, c, host, fb, ranges, cap, base, time_major):
    """Stitch the given (g0, N) ranges of `host` into one canary-filled buffer of cap frames; return the whole
    buffer from the device and what it must hold."""
    buf, off = offset_buffer(cap * fb, fill=CANARY)
    out = buf[off:off + cap * fb].view(cap, fb)
    assert out.data_ptr() % 16 == 2
    want = np.full(buf.numel(), CANARY, np.uint8)
    canvas = want[off:off + cap * fb].reshape(cap, fb)
    for g0, n in ranges:
        rows = device_rows(host[g0:g0 + n], time_major)
        got = codec.stitch(c.plan, rows, first_segment=g0, out=out, frame_base=base, time_major=time_major)
        assert got.data_ptr() == out.data_ptr()
        ref_gather(canvas, c.want_plan, host[g0:g0 + n], g0, base)
    return buf.cpu().numpy(), want, off


def assert_same_bytes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: got {got[bad[0]]:#x}, "
                             f"want {want[bad[0]]:#x}")


def model_output(c, fb, seed=0):
    rng = np.random.default_rng(fb + seed)
    return rng.integers(0, 256, (c.total, c.T, fb), dtype=np.uint8)


@pytest.mark.parametrize("time_major", [False, True], ids=["NTC", "TNC"])
@pytest.mark.parametrize("fb", FRAME_BYTES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=str)
def test_rows_whole_table(codec, cases, cfg, fb, time_major):
    """The whole table at once, rows and output 2 bytes off a 16-byte boundary, two spare frames of capacity:
    every byte of the output and of the canaries around it."""
    c = cases(cfg)
    host = model_output(c, fb)
    got, want, _ = run_rows(codec, c, host, fb, [(0, c.total)], c.frames + 2, 0, time_major)
    assert_same_bytes(got, want, f"{cfg} fb={fb} time_major={time_major}")


@pytest.mark.parametrize("time_major", [False, True], ids=["NTC", "TNC"])
@pytest.mark.parametrize("fb", [6, 16])
def test_rows_in_batches_of_seven(codec, cases, fb, time_major):
    """The first 700 table rows in batches of 7, which split reads mid-way, into one output: what one call for
    the 700 rows gives."""
    c = cases((40, 7, 4))
    host = model_output(c, fb, 1)[:700]
    cap = int(c.want_plan["dst_frame"][700])
    assert cap > 0 and (c.reads["nsegments"] > 7).any()
    batches = [(g, min(7, 700 - g)) for g in range(0, 700, 7)]
    got, want, _ = run_rows(codec, c, host, fb, batches, cap, 0, time_major)
    assert_same_bytes(got, want, "batches")
    once, _, _ = run_rows(codec, c, host, fb, [(0, 700)], cap, 0, time_major)
    assert_same_bytes(got, once, "batches against one call")


@pytest.mark.parametrize("time_major", [False, True], ids=["NTC", "TNC"])
@pytest.mark.parametrize("fb", [2, 16, 18])
def test_rows_range_into_its_own_buffer(codec, cases, fb, time_major):
    """Rows [g0, g0 + 50) with out_frame_base at their first dst_frame into a buffer of just their frames; the
    same one frame short, where only the last frame is missing; and a base three frames further on, which cuts
    into the first row's frames."""
    c = cases((48, 12, 6))
    g0 = int(c.reads["first_segment"][c.reads["nsegments"].argmax()]) + 5  # inside the long read
    host = np.zeros((c.total, c.T, fb), np.uint8)
    host[g0:g0 + 50] = model_output(c, fb, 2)[g0:g0 + 50]
    base = int(c.want_plan["dst_frame"][g0])
    n = int(c.want_plan["dst_frame"][g0 + 50]) - base
    assert base > 0 and n > 50
    full, want, off = run_rows(codec, c, host, fb, [(g0, 50)], n, base, time_major)
    assert_same_bytes(full, want, "own buffer")
    short, want_short, off_short = run_rows(codec, c, host, fb, [(g0, 50)], n - 1, base, time_major)
    assert_same_bytes(short, want_short, "one frame short")
    k = off + (n - 1) * fb  # the same bytes up to the missing frame, canaries from there on
    assert off_short == off and np.array_equal(short[:k], full[:k]) and (short[k:] == CANARY).all()
    cut, want_cut, _ = run_rows(codec, c, host, fb, [(g0, 50)], n, base + 3, time_major)
    assert_same_bytes(cut, want_cut, "base inside a row")
    assert c.want_plan["count"][g0] > 3


def test_rows_python_argument_validation(codec, cases):
    import torch

    c = cases((40, 7, 4))
    rows = torch.zeros((4, c.T, 3), dtype=torch.float16, device="cuda:0")
    out = torch.zeros((100, 3), dtype=torch.float16, device="cuda:0")
    codec.stitch(c.plan, rows, out=out)
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows[:, :-1], out=out)                    # T
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows, out=out.to(torch.float32))          # dtype
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows, out=out[:, :2])                     # frame shape
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows[:, :, ::2], out=out[:, :2].contiguous())  # a strided frame
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows, first_segment=c.total + 10_000, out=out)
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows.cpu(), out=out)
    with pytest.raises(ValueError):
        codec.stitch(c.plan, rows, out=out, time_major=True)
    whole = codec.stitch(c.plan, torch.zeros((c.total, c.T), dtype=torch.int16, device="cuda:0"))
    assert tuple(whole.shape) == (c.frames,)


def test_pod5_fixture_identity_model(codec):
    """Pod5File.load_segments on the committed file, an identity "model" of stride s (row j's frame f is its
    samples [f*s, f*s + s)), stitched: every kept frame is the trimmed, normalised read at the frame's first
    sample (from segment_signal on the CPU oracle's decode), the frames are those of the numpy rule, and where
    the read ends on the segment grid or fits one row the frames laid end to end are the read itself."""
    import torch

    from _golden import HERE as GOLDEN, real_vbz_chunks
    from rawnanoporesignalcompression_amd import segment_signal, stitch_bound
    from rawnanoporesignalcompression_amd.pod5_file import Pod5File
    from test_gpu_pod5_reads import LISTS
    from test_norm_api import QUANTILE

    chunks = []
    for blob, n in real_vbz_chunks():
        rc, x = O.vbz_decompress(blob, n)
        assert rc == 0
        chunks.append(x.copy())
    reads = [np.concatenate([chunks[k] for k in lst]) for lst in LISTS]
    L, V, s = 1000, 100, 5
    T, S = L // s, L - V
    with Pod5File(os.path.join(GOLDEN, "multi_fast5_zip_v3.pod5")) as f:
        res = f.load_segments(codec, length=L, overlap=V, trim=True, dtype=torch.float16, **QUANTILE)
    plan = codec.stitch_plan(res, L, V, s)
    total = int(res.total.item())
    out = codec.stitch(plan, res.out[:total].view(total, T, s))
    rtab, stab = res.reads.numpy(), res.segments.numpy()
    want_plan, want_frames = ref_tables(rtab, stab, len(stab), L, V, s)
    check_plan(plan, want_plan, want_frames, "pod5")
    assert tuple(out.shape) == (int(want_frames[-1]), s) and out.dtype == torch.float16
    assert out.shape[0] <= stitch_bound([r.size for r in reads], L, V, s)
    got = out.cpu().numpy().view(np.uint16)
    exact = 0
    for r, x in enumerate(reads):
        rows = segment_signal(x, L, V, trim=True, dtype=np.float16, **QUANTILE)
        first, k, trim = int(rtab["first_segment"][r]), int(rtab["nsegments"][r]), int(rtab["trim"][r])
        assert rows.shape[0] == k and k > 0
        m = x.size - trim
        z = np.zeros(max(m, L) + s, np.float16)  # the trimmed, normalised read, +0.0 behind it as in a short row
        for j in range(k):
            a = int(stab["start"][first + j]) - trim
            z[a:a + L] = rows[j]
        mine = got[want_frames[r]:want_frames[r + 1]]
        pos = np.concatenate([int(stab["start"][first + j]) - trim + s * np.arange(p["first"], p["first"] + p["count"])
                              for j, p in enumerate(want_plan[first:first + k])])
        want = z.view(np.uint16)[pos[:, None] + np.arange(s)[None, :]]
        assert np.array_equal(mine, want), f"read {r}"
        if k == 1 or (m - L) % S == 0:
            exact += 1
            assert mine.shape[0] == -(-m // s) and np.array_equal(mine.reshape(-1)[:m], z.view(np.uint16)[:m]), f"read {r}"
        else:  # the regular joints still tile: up to the last row's first kept frame the frames are the read
            upto = int(want_frames[r + 1] - want_frames[r] - want_plan["count"][first + k - 1]) * s
            assert np.array_equal(mine.reshape(-1)[:upto], z.view(np.uint16)[:upto]), f"read {r}"
    print("reads whose stitched frames are the whole read:", exact, "of", len(reads))
