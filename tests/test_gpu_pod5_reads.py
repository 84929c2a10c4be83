"""Whole reads of a POD5 file on the device (Pod5File.load_reads -> pgn_pod5_load_reads_device /
pgn_pod5_load_row_lists_device, and pgn_decompress_reads_device_pa under them).

Data: the committed fixture only (10 reads, 22 signal rows, 1.55 M samples) as three files of the same
content -- the fixture itself (VBZ), its pgnano transcode, and an uncompressed copy written from the
golden rows.  The expected samples come from the CPU oracle's decode of the golden VBZ rows (their
SHA-256 is pinned in c5_golden.json); pA and the normalised values from the numpy references of
tests/test_decode_pa_api.py and tests/test_norm_api.py.  Every comparison is of bit patterns."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import _oracle as O
from _golden import HERE as GOLDEN, golden, real_vbz_chunks
from test_norm_api import MEDMAD, QUANTILE, assert_stats_equal, ref_norm, ref_stats

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "multi_fast5_zip_v3.pod5")
LISTS = [[0, 1], [2], [3, 4, 5, 6], [7, 8], [9, 10, 11, 12, 13], [14, 15, 16], [17], [18], [19, 20], [21]]
KINDS = ["vbz", "pgnano", "uncompressed"]
DST_TOO_SMALL, UNSUPPORTED, INVALID_ARG = 1, 9, 10


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:1]}"


@pytest.fixture(scope="module")
def rows_signal():
    """The 22 rows' samples from the CPU oracle (checked against the pinned digests)."""
    g = golden()
    out = []
    for i, (blob, n) in enumerate(real_vbz_chunks()):
        rc, x = O.vbz_decompress(blob, n)
        assert rc == 0 and hashlib.sha256(x.tobytes()).hexdigest() == g["real"][i]["signal_sha256"]
        out.append(x.copy())
    return out


@pytest.fixture(scope="module")
def truth(rows_signal):
    """Per read: the samples, the calibration, and the statistics of both modes (computed once)."""
    from rawnanoporesignalcompression_amd.pod5_file import Pod5File

    with Pod5File(FIXTURE) as f:
        t = f.reads()
    sig = [np.concatenate([rows_signal[k] for k in rows]) for rows in LISTS]
    assert [s.size for s in sig] == t.signal_samples.tolist()
    stats = {"quantile": [ref_stats(s, **QUANTILE) for s in sig], "medmad": [ref_stats(s, **MEDMAD) for s in sig]}
    return dict(sig=sig, off=t.calibration_offset, scale=t.calibration_scale, stats=stats, table=t)


@pytest.fixture(scope="module")
def files(codec, rows_signal, tmp_path_factory):
    from rawnanoporesignalcompression_amd.pod5_file import Pod5File, SignalTable, transcode_pod5, write_pod5

    d = tmp_path_factory.mktemp("pod5_reads")
    pg, unc, bare = str(d / "pgnano.pod5"), str(d / "unc.pod5"), str(d / "bare.pod5")
    transcode_pod5(FIXTURE, pg, "pgnano", codec=codec)
    with Pod5File(FIXTURE) as f:
        ids, samples = f.row_columns()
        assert samples.tolist() == [x.size for x in rows_signal]
        offs = np.zeros(23, np.uint64)
        np.cumsum(2 * samples.astype(np.uint64), out=offs[1:])
        data = np.concatenate(rows_signal).astype("<i2").view(np.uint8)
        write_pod5(unc, SignalTable(ids, samples, offs, data, "uncompressed"), source=f, rows_per_batch=4)
        write_pod5(bare, f.signal_table(), source=None)  # VBZ rows, no reads table
    opened = {"vbz": Pod5File(FIXTURE), "pgnano": Pod5File(pg), "uncompressed": Pod5File(unc), "bare": Pod5File(bare)}
    assert [opened[k].signal_type for k in KINDS] == KINDS
    yield opened
    for f in opened.values():
        f.close()


def read_of(res, r):
    o, n = int(res.offsets[r]), int(res.counts[r])
    return res.out[o:o + n].cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_adc_and_pa_are_the_golden_reads(codec, files, truth, kind):
    import torch

    from rawnanoporesignalcompression_amd import calibrate_signal

    f = files[kind]
    for output, dtype, npdt in (("adc", torch.int16, np.int16), ("pa", torch.float32, np.float32),
                                ("pa", torch.float16, np.float16)):
        res = f.load_reads(codec, output=output, dtype=dtype)
        torch.cuda.synchronize()
        assert res.status.cpu().tolist() == [0] * 10 and res.stats is None
        assert res.counts.tolist() == [s.size for s in truth["sig"]]
        assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(res.counts)[:-1]]).tolist()
        assert res.out.dtype == dtype and res.out.numel() == int(res.counts.sum())
        for r, s in enumerate(truth["sig"]):
            want = s if output == "adc" else calibrate_signal(s, truth["off"][r], truth["scale"][r], npdt)
            same_bits(read_of(res, r), want, f"{kind} {output} {npdt.__name__} read {r}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params", [QUANTILE, MEDMAD], ids=["quantile", "medmad"])
def test_norm_is_the_reference(codec, files, truth, kind, params):
    import torch

    f = files[kind]
    want_stats = truth["stats"][params["mode"]]
    for dtype, npdt in ((torch.float16, np.float16), (torch.float32, np.float32)):
        res = f.load_reads(codec, output="norm", dtype=dtype, **params)
        torch.cuda.synchronize()
        assert res.status.cpu().tolist() == [0] * 10
        got = res.stats.numpy()
        for r, s in enumerate(truth["sig"]):
            assert_stats_equal(got[r], want_stats[r], f"{kind} read {r}")
            same_bits(read_of(res, r), ref_norm(s, want_stats[r]["centre"], want_stats[r]["spread"], npdt),
                      f"{kind} {params['mode']} {npdt.__name__} read {r}")
        if dtype == torch.float32:  # the workspace allocated by load_reads holds the raw samples
            o, n = int(res.offsets[4]), int(res.counts[4])
            same_bits(res.adc[o:o + n].cpu().numpy(), truth["sig"][4], "adc workspace")


@pytest.mark.parametrize("kind", KINDS)
def test_selection_repeats_and_order(codec, files, truth, kind):
    import torch

    from rawnanoporesignalcompression_amd import calibrate_signal

    sel = [4, 0, 4, 9]
    t = truth["table"]
    res = files[kind].load_reads(codec, reads=t.index_of([bytes(t.read_id[i]) for i in sel]), output="pa", dtype=torch.float16)
    torch.cuda.synchronize()
    assert res.counts.tolist() == [truth["sig"][r].size for r in sel]
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(res.counts)[:-1]]).tolist()
    assert res.status.cpu().tolist() == [0] * 4
    for k, r in enumerate(sel):
        same_bits(read_of(res, k), calibrate_signal(truth["sig"][r], truth["off"][r], truth["scale"][r], np.float16), f"{kind} {k}")
    res = files[kind].load_reads(codec, reads=[4, 0, 4, 9], output="norm", dtype=torch.float16, **QUANTILE)
    torch.cuda.synchronize()
    for k, r in enumerate(sel):
        st = truth["stats"]["quantile"][r]
        assert_stats_equal(res.stats.numpy()[k], st, f"{kind} {k}")
        same_bits(read_of(res, k), ref_norm(truth["sig"][r], st["centre"], st["spread"], np.float16), f"{kind} norm {k}")


@pytest.mark.parametrize("kind", KINDS)
def test_empty_selection(codec, files, kind):
    import torch

    for output in ("adc", "pa", "norm"):
        res = files[kind].load_reads(codec, reads=[], output=output)
        torch.cuda.synchronize()
        assert res.offsets.size == 0 and res.counts.size == 0 and res.status.numel() == 0


@pytest.mark.parametrize("kind", KINDS)
def test_odd_offsets_with_gaps_leave_the_gaps_alone(codec, files, truth, kind):
    """Reads at 2-byte-aligned-only places (odd element offsets for the 2-byte types) with gaps of 1 to 9
    elements between them: the gaps, the head and everything past the last read keep a sentinel."""
    import torch

    from rawnanoporesignalcompression_amd import calibrate_signal

    sel = [6, 2, 7, 0, 9]
    counts = [truth["sig"][r].size for r in sel]
    offs, at = [], 1
    for k, n in enumerate(counts):
        offs.append(at)
        at += n + 1 + k
        at += 1 - at % 2  # the next start is odd again
    total = offs[-1] + counts[-1] + 37
    assert all(o % 2 == 1 for o in offs)
    for output, dtype, npdt, fill in (("adc", torch.int16, np.int16, 0x5A5A), ("pa", torch.float16, np.float16, 0x7E01),
                                      ("pa", torch.float32, np.float32, 0x7FC00123), ("norm", torch.float16, np.float16, 0x7E01)):
        sentinel = np.full(total, fill, {2: np.uint16, 4: np.uint32}[np.dtype(npdt).itemsize])
        out = torch.from_numpy(sentinel.view(npdt).copy()).cuda()
        kw = dict(QUANTILE) if output == "norm" else {}
        res = files[kind].load_reads(codec, reads=sel, output=output, dtype=dtype, out=out, out_offsets=offs, **kw)
        torch.cuda.synchronize()
        assert res.out is out and res.offsets.tolist() == offs and res.counts.tolist() == counts
        got = out.cpu().numpy()
        covered = np.zeros(total, bool)
        for k, r in enumerate(sel):
            s = truth["sig"][r]
            if output == "adc":
                want = s
            elif output == "pa":
                want = calibrate_signal(s, truth["off"][r], truth["scale"][r], npdt)
            else:
                st = truth["stats"]["quantile"][r]
                want = ref_norm(s, st["centre"], st["spread"], npdt)
            same_bits(got[offs[k]:offs[k] + counts[k]], want, f"{kind} {output} read {r}")
            covered[offs[k]:offs[k] + counts[k]] = True
        assert (bits(got)[~covered] == fill).all(), f"{kind} {output}: a write outside the reads"


def _c_load(codec, f, first, rows, cal, args, lists=True, index=None, nreads=None):
    lib = codec._lib
    if lists:
        return lib.pgn_pod5_load_row_lists_device(codec._h, f._h, len(first) - 1, first.ctypes.data,
                                                  rows.ctypes.data if rows.size else None,
                                                  cal[0].ctypes.data if cal else None, cal[1].ctypes.data if cal else None,
                                                  C.byref(args), None)
    return lib.pgn_pod5_load_reads_device(codec._h, f._h, index.ctypes.data, nreads, C.byref(args), None)


def test_refusals_come_before_any_launch(codec, files, truth):
    import torch

    from rawnanoporesignalcompression_amd import PGNanoError, _native, norm_params

    f = files["vbz"]
    need = truth["sig"][0].size + truth["sig"][1].size
    out = torch.full((need,), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(PGNanoError) as e:
        f.load_reads(codec, reads=[0, 1], output="adc", out=out[:need - 1])
    assert e.value.status == DST_TOO_SMALL
    with pytest.raises(PGNanoError) as e:
        f.load_reads(codec, reads=[0, 1], output="adc", out=out, out_offsets=[0, truth["sig"][0].size + 1])
    assert e.value.status == DST_TOO_SMALL
    torch.cuda.synchronize()
    assert (out == 0x5A5A).all()  # nothing ran
    # the C calls' own checks (the Python layer refuses these before it calls)
    A = _native.LoadArgs
    adc_args = A(_native.PGN_LOAD_ADC, _native.PGN_OUT_INT16, 0, 0, None, out.data_ptr(), need, None, None, None, None, None, None)
    one = np.array([0, 1], np.uint64)
    assert _c_load(codec, f, None, None, None, adc_args, lists=False, index=np.array([10], np.uint64), nreads=1) == INVALID_ARG
    assert _c_load(codec, f, one, np.array([22], np.uint64), None, adc_args) == INVALID_ARG
    assert _c_load(codec, f, np.array([1, 0], np.uint64), np.array([0], np.uint64), None, adc_args) == INVALID_ARG
    bad_type = A(_native.PGN_LOAD_ADC, _native.PGN_OUT_F32, 0, 0, None, out.data_ptr(), need, None, None, None, None, None, None)
    assert _c_load(codec, f, one, np.array([2], np.uint64), None, bad_type) == INVALID_ARG
    bad_kind = A(3, _native.PGN_OUT_INT16, 0, 0, None, out.data_ptr(), need, None, None, None, None, None, None)
    assert _c_load(codec, f, one, np.array([2], np.uint64), None, bad_kind) == INVALID_ARG
    pa_args = A(_native.PGN_LOAD_PA, _native.PGN_OUT_F16, 0, 0, None, out.data_ptr(), need, None, None, None, None, None, None)
    assert _c_load(codec, f, one, np.array([2], np.uint64), None, pa_args) == INVALID_ARG  # no calibration
    prm = norm_params(**QUANTILE)
    f32 = torch.zeros(need, dtype=torch.float32, device="cuda")
    norm_args = A(_native.PGN_LOAD_NORM, _native.PGN_OUT_F32, 0, 0, C.pointer(prm), f32.data_ptr(), need, None, None, None, None,
                  None, None)
    assert _c_load(codec, f, one, np.array([2], np.uint64), None, norm_args) == INVALID_ARG  # float32 without d_adc
    bad_prm = norm_params(**dict(QUANTILE, spread_floor=0.0))
    norm_args = A(_native.PGN_LOAD_NORM, _native.PGN_OUT_F16, 0, 0, C.pointer(bad_prm), out.data_ptr(), need, None, None, None,
                  None, None, None)
    assert _c_load(codec, f, one, np.array([2], np.uint64), None, norm_args) == INVALID_ARG
    bad_variant = A(_native.PGN_LOAD_ADC, _native.PGN_OUT_INT16, 17, 0, None, out.data_ptr(), need, None, None, None, None, None, None)
    assert _c_load(codec, files["pgnano"], one, np.array([2], np.uint64), None, bad_variant) == INVALID_ARG
    assert codec._lib.pgn_pod5_load_reads_device(None, f._h, None, 0, C.byref(adc_args), None) == INVALID_ARG
    assert _c_load(codec, files["bare"], None, None, None, adc_args, lists=False, index=np.array([0], np.uint64), nreads=1) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 0x5A5A).all() and (f32 == 0).all()
    with pytest.raises(ValueError):
        f.load_reads(codec, reads=[10])
    with pytest.raises(ValueError):
        f.load_reads(codec, output="adc", dtype=torch.float32)
    with pytest.raises(ValueError):
        f.load_reads(codec, output="pa", spread_floor=2.0)


def test_row_lists_on_a_file_without_reads_table(codec, files, truth):
    import torch

    t = truth["table"]
    for output, dtype, kw in (("pa", torch.float16, {}), ("adc", torch.int16, {}), ("norm", torch.float32, MEDMAD)):
        want = files["vbz"].load_reads(codec, output=output, dtype=dtype, **kw)
        got = files["bare"].load_reads(codec, output=output, dtype=dtype, row_lists=(t.row_first, t.rows),
                                       calibration=(t.calibration_offset, t.calibration_scale), **kw)
        torch.cuda.synchronize()
        assert got.offsets.tolist() == want.offsets.tolist() and got.counts.tolist() == want.counts.tolist()
        same_bits(got.out.cpu().numpy(), want.out.cpu().numpy(), output)
        assert got.status.cpu().tolist() == [0] * 10
    # a sub-range of the lists (row_first need not start at 0), calibration optional for adc
    got = files["bare"].load_reads(codec, output="adc", row_lists=(t.row_first[2:5], t.rows))
    torch.cuda.synchronize()
    same_bits(got.out.cpu().numpy(), np.concatenate(truth["sig"][2:4]), "sub-range")


@pytest.mark.parametrize("kind", ["vbz", "pgnano"])
def test_a_damaged_row_fails_its_read_only(codec, files, truth, kind, tmp_path):
    import torch

    from rawnanoporesignalcompression_amd import VBZCodec
    from rawnanoporesignalcompression_amd.pod5_file import Pod5File, write_pod5

    src = files[kind]
    t = src.signal_table()
    lo, hi = int(t.offsets[4]), int(t.offsets[5])
    # a byte of row 4's (first) zstd frame, its magic number -- a flip in the middle of a frame often
    # still decodes, to other samples; read 2 lists rows 3..6
    t.data[lo + (0 if kind == "vbz" else 8)] ^= 0x5A
    p = str(tmp_path / "damaged.pod5")
    write_pod5(p, t, source=src)
    # what the batch decode makes of that blob
    dec = VBZCodec(0) if kind == "vbz" else codec
    try:
        blob = torch.from_numpy(t.data[lo:hi].copy()).cuda()
        _, _, st = dec.decompress_batch(blob, torch.tensor([0]), torch.tensor([hi - lo]), torch.tensor([int(t.samples[4])]))
        torch.cuda.synchronize()
        want_status = int(st.cpu()[0])
    finally:
        if dec is not codec:
            dec.close()
    counts = [s.size for s in truth["sig"]]
    offs = [3 + sum(counts[:r]) + 5 * r for r in range(10)]
    total = offs[-1] + counts[-1] + 11
    out = torch.full((total,), 0x5A5A, dtype=torch.int16, device="cuda")
    with Pod5File(p) as f:
        res = f.load_reads(codec, output="adc", out=out, out_offsets=offs)
        torch.cuda.synchronize()
    status = res.status.cpu().tolist()
    assert status[2] == want_status and status[:2] + status[3:] == [0] * 9
    assert want_status != 0
    got = out.cpu().numpy()
    covered = np.zeros(total, bool)
    for r in range(10):
        covered[offs[r]:offs[r] + counts[r]] = True
        if r != 2:
            same_bits(got[offs[r]:offs[r] + counts[r]], truth["sig"][r], f"read {r}")
    assert (got[~covered] == 0x5A5A).all()


# ---- pgn_decompress_reads_device_pa against pgn_decompress_batch_device_pa ------------------------
COUNTS = [1000, 0, 1, 1, 4096, 300, 70001, 263000, 17]
FIRST = [0, 2, 2, 3, 4, 7, 8, 8, 9]  # read 1 and read 6 have no chunks; reads 2 and 3 have one sample


@pytest.fixture(scope="module", params=["C5", "VBZ", "C3"])
def variant_codec(request):
    from rawnanoporesignalcompression_amd import PGNanoCodec, VBZCodec

    c = VBZCodec(0) if request.param == "VBZ" else PGNanoCodec(0, request.param)
    yield c
    c.close()


@pytest.mark.parametrize("bound", [0, 263000], ids=["unbounded", "bounded"])
def test_reads_pa_is_batch_pa_with_the_arrays_expanded(variant_codec, bound):
    import torch

    c = variant_codec
    samples, offs, cnt = c.synth_reads(len(COUNTS), COUNTS, seed=7)
    enc = c.compress_batch(samples, offs, cnt)
    torch.cuda.synchronize()
    assert (enc.status == 0).all()
    nreads = len(FIRST) - 1
    rng = np.random.default_rng(5)
    cal_off = rng.integers(-300, 300, nreads).astype(np.float32) + np.float32(0.25)
    cal_scale = rng.uniform(0.05, 0.4, nreads).astype(np.float32)
    read_of_chunk = np.repeat(np.arange(nreads), np.diff(FIRST))
    n_read = [sum(COUNTS[FIRST[r]:FIRST[r + 1]]) for r in range(nreads)]
    read_off, at = [], 1
    for n in n_read:  # gaps, odd starts
        read_off.append(at)
        at += n + 3
    chunk_off = []
    for r in range(nreads):
        acc = read_off[r]
        for k in range(FIRST[r], FIRST[r + 1]):
            chunk_off.append(acc)
            acc += COUNTS[k]
    total = at + 8
    for dtype, fill in ((torch.int16, 0x5A5A), (torch.float32, 0x7FC00123), (torch.float16, 0x7E01)):
        npdt = {torch.int16: np.int16, torch.float32: np.float32, torch.float16: np.float16}[dtype]
        sent = np.full(total, fill, {2: np.uint16, 4: np.uint32}[np.dtype(npdt).itemsize]).view(npdt)
        want, got = torch.from_numpy(sent.copy()).cuda(), torch.from_numpy(sent.copy()).cuda()
        cal = dtype != torch.int16
        _, _, wst = c.decompress_batch_pa(enc.blobs, enc.offsets, enc.sizes, cnt,
                                          torch.from_numpy(cal_off[read_of_chunk]) if cal else None,
                                          torch.from_numpy(cal_scale[read_of_chunk]) if cal else None, dtype=dtype, out=want,
                                          out_offsets=torch.tensor(chunk_off), max_chunk_samples=bound or None)
        _, ro, rst, cst = c.decompress_reads_pa(enc.blobs, enc.offsets, enc.sizes, cnt, torch.tensor(FIRST),
                                                torch.from_numpy(cal_off) if cal else None,
                                                torch.from_numpy(cal_scale) if cal else None, dtype=dtype, out=got,
                                                read_out_offsets=torch.tensor(read_off), max_chunk_samples=bound)
        torch.cuda.synchronize()
        assert cst.cpu().tolist() == wst.cpu().tolist() == [0] * len(COUNTS)
        assert rst.cpu().tolist() == [0] * nreads and ro.cpu().tolist() == read_off
        same_bits(got.cpu().numpy(), want.cpu().numpy(), f"{dtype}")
        x = samples.cpu().numpy()
        if dtype == torch.int16:  # and the decode is the encoder's input
            k = 6
            same_bits(got.cpu().numpy()[chunk_off[k]:chunk_off[k] + COUNTS[k]], x[int(offs[k]):int(offs[k]) + COUNTS[k]], "chunk 6")


def test_reads_pa_statuses_and_empty_calls(variant_codec):
    import torch

    c = variant_codec
    samples, offs, cnt = c.synth_reads(len(COUNTS), COUNTS, seed=9)
    enc = c.compress_batch(samples, offs, cnt)
    torch.cuda.synchronize()
    blobs = enc.blobs.clone()
    sizes = enc.sizes.clone()
    sizes[4] -= 9                                     # read 4's first chunk: truncated
    mid = int(enc.offsets[8]) + int(enc.sizes[8]) // 2
    blobs[mid] ^= 0x5A                                # read 7's only chunk: a flipped byte
    _, _, want = c.decompress_batch(blobs, enc.offsets, sizes, cnt)
    out, _, rst, cst = c.decompress_reads_pa(blobs, enc.offsets, sizes, cnt, torch.tensor(FIRST), dtype=torch.int16)
    torch.cuda.synchronize()
    want, cst = want.cpu().tolist(), cst.cpu().tolist()
    assert cst == want and want[4] != 0
    expect = [next((want[k] for k in range(FIRST[r], FIRST[r + 1]) if want[k]), 0) for r in range(len(FIRST) - 1)]
    assert rst.cpu().tolist() == expect and expect[4] == want[4] and expect[1] == 0 and expect[6] == 0
    assert c.reads_status(torch.tensor(FIRST), torch.tensor(want, dtype=torch.int32).cuda()).cpu().tolist() == expect
    # no reads at all, and reads without a single chunk
    e8, e4 = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    out, ro, rst, cst = c.decompress_reads_pa(blobs[:0], e8, e8, e4, torch.tensor([0]), dtype=torch.int16)
    assert ro.numel() == 0 and rst.numel() == 0 and cst.numel() == 0
    out, ro, rst, cst = c.decompress_reads_pa(blobs[:0], e8, e8, e4, torch.tensor([0, 0, 0]), torch.zeros(2), torch.ones(2),
                                              dtype=torch.float16)
    torch.cuda.synchronize()
    assert rst.cpu().tolist() == [0, 0] and ro.cpu().tolist() == [0, 0]
    with pytest.raises(ValueError):
        c.decompress_reads_pa(blobs, enc.offsets, sizes, cnt, torch.tensor(FIRST), torch.zeros(3), torch.ones(3))
    with pytest.raises(ValueError):
        c.decompress_reads_pa(blobs, enc.offsets, sizes, cnt, torch.tensor(FIRST), dtype=torch.float64)
    with pytest.raises(ValueError):
        c.decompress_reads_pa(blobs.cpu(), enc.offsets, sizes, cnt, torch.tensor(FIRST), dtype=torch.int16)
