"""The reads table of a POD5 file without Arrow (pgn_pod5_reads_info / pgn_pod5_reads_read,
include/pgnano_pod5file.h), CPU only.

What the reference's reader gives through pod5_get_read_batch_row_info_data, pod5_get_signal_row_indices
and pod5_get_read_complete_sample_count (pod5/c++/pod5_format/c_api.h:315-350, 489-502).  Pinned by the
committed fixture (the values below were read from it with pyarrow 25) and, where pyarrow is
installed, by pyarrow's reading of the same embedded Arrow file.

The reference's older fixtures, multi_fast5_zip_v{0,1,2}.pod5 (read where the reference is mounted), all
give PGN_ERR_UNSUPPORTED: v0 and v1 name `num_samples` (the first flat column they lack), v2 names
`calibration_offset` (it has `num_samples`; its calibration is still a dictionary struct)."""
import ctypes as C
import os
import shutil
import subprocess
import uuid

import numpy as np
import pytest

from _golden import HERE as GOLDEN

from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd import pod5_file as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN, "multi_fast5_zip_v3.pod5")
REF_DATA = "/root/reference/pod5/test_data"
UNSUPPORTED, CORRUPT = _native.PGN_ERR_UNSUPPORTED, _native.PGN_ERR_CORRUPT

SIGNAL_LISTS = [[0, 1], [2], [3, 4, 5, 6], [7, 8], [9, 10, 11, 12, 13], [14, 15, 16], [17], [18], [19, 20], [21]]
SAMPLES = [123627, 37440, 337876, 161547, 505057, 206976, 14510, 9885, 136370, 15643]
CAL_OFFSET = [21, 4, 6, 2, 23, 4, 5, 2, 37, 14]
SCALE_BITS = 0x3E33B653  # calibration_scale of every read: float32 0.17550019919872284


def lists_of(t):
    return [t.rows[int(t.row_first[r]):int(t.row_first[r + 1])].tolist() for r in range(len(t))]


def reads_range(path):
    with P.Pod5File(path) as f:
        return [(o, ln) for n, o, ln in f.embedded if n == "reads"][0]


def arrow_reads(path):
    pa = pytest.importorskip("pyarrow")
    ipc = pytest.importorskip("pyarrow.ipc")
    raw = open(path, "rb").read()
    o, ln = reads_range(path)  # from pgn_pod5_file_embedded
    return ipc.open_file(pa.BufferReader(raw[o:o + ln]))


def assert_equals_arrow(t, path):
    r = arrow_reads(path)
    a = r.read_all()
    assert len(t) == a.num_rows
    assert [bytes(t.read_id[i]) for i in range(len(t))] == [bytes(v) for v in a.column("read_id").to_pylist()]
    assert lists_of(t) == a.column("signal").to_pylist()
    for ours, name, dt in ((t.num_samples, "num_samples", np.uint64), (t.read_number, "read_number", np.uint32),
                           (t.channel, "channel", np.uint16), (t.well, "well", np.uint8)):
        assert ours.dtype == dt and ours.tolist() == a.column(name).to_pylist(), name
    for ours, name in ((t.calibration_offset, "calibration_offset"), (t.calibration_scale, "calibration_scale")):
        want = np.asarray(a.column(name).to_numpy(), np.float32)
        assert ours.dtype == np.float32 and np.array_equal(ours.view(np.uint32), want.view(np.uint32)), name
    return r.num_record_batches


def test_fixture_reads_table_is_the_recorded_one():
    with P.Pod5File(FIXTURE) as f:
        t = f.reads()
        _, samples = f.row_columns()
    assert len(t) == 10 and t.rows.size == 22 and t.row_first.tolist() == [0, 2, 3, 7, 9, 14, 17, 18, 19, 21, 22]
    assert lists_of(t) == SIGNAL_LISTS
    assert t.signal_samples.tolist() == SAMPLES and t.num_samples.tolist() == SAMPLES
    assert t.signal_samples.tolist() == [int(samples[rows].sum()) for rows in SIGNAL_LISTS]
    assert t.calibration_offset.tolist() == CAL_OFFSET
    assert t.calibration_scale.view(np.uint32).tolist() == [SCALE_BITS] * 10  # one run: one scale
    assert t.read_id.shape == (10, 16) and len({bytes(r) for r in t.read_id}) == 10


def test_fixture_reads_table_against_pyarrow():
    with P.Pod5File(FIXTURE) as f:
        t = f.reads()
        assert assert_equals_arrow(t, FIXTURE) == t.batches == 1


def test_every_null_pointer_combination():
    lib = _native.load()
    with P.Pod5File(FIXTURE) as f:
        t = f.reads()
        full = [t.read_id, t.row_first, t.rows, t.num_samples, t.signal_samples, t.calibration_offset,
                t.calibration_scale, t.read_number, t.channel, t.well]
        for info_mask in range(8):
            n, nb, ne = C.c_uint64(), C.c_uint32(), C.c_uint64()
            assert lib.pgn_pod5_reads_info(f._h, C.byref(n) if info_mask & 1 else None, C.byref(nb) if info_mask & 2 else None,
                                           C.byref(ne) if info_mask & 4 else None) == 0
            assert (n.value, nb.value, ne.value) == (10 * (info_mask & 1), (info_mask >> 1) & 1, 22 * ((info_mask >> 2) & 1))
        for mask in range(1 << len(full)):
            got = [np.full_like(a, 0xA5 if a.dtype == np.uint8 else 7) for a in full]
            args = [g.ctypes.data if mask >> i & 1 else None for i, g in enumerate(got)]
            assert lib.pgn_pod5_reads_read(f._h, *args) == 0
            for i, (g, a) in enumerate(zip(got, full)):
                if mask >> i & 1:
                    assert g.tobytes() == a.tobytes(), (mask, i)
                else:  # a skipped array is not touched
                    assert (g == (0xA5 if a.dtype == np.uint8 else 7)).all(), (mask, i)
    assert lib.pgn_pod5_reads_info(None, None, None, None) == _native.PGN_ERR_INVALID_ARG
    assert lib.pgn_pod5_reads_read(*[None] * 11) == _native.PGN_ERR_INVALID_ARG


def test_c_abi_exports_and_structs():
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "pgnano_pod5file.h")).read()
    hip = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs, src in (("pgn_pod5_reads_info", 4, header), ("pgn_pod5_reads_read", 11, header),
                             ("pgn_pod5_load_row_lists_device", 9, header), ("pgn_pod5_load_reads_device", 6, header),
                             ("pgn_decompress_reads_device_pa", 18, hip), ("pgn_reads_status_device", 6, hip)):
        assert ("int " + name + "(") in src
        assert hasattr(lib, name) and sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs, name
    # pgn_pod5_load_args: four int32, then eight pointers and one uint64, no padding
    assert C.sizeof(_native.LoadArgs) == 16 + 9 * 8
    assert _native.LoadArgs.d_out.offset == 24 and _native.LoadArgs.out_capacity.offset == 32
    assert _native.LoadArgs.read_counts_out.offset == 80
    assert (_native.PGN_LOAD_ADC, _native.PGN_LOAD_PA, _native.PGN_LOAD_NORM) == (0, 1, 2)
    assert "typedef enum { PGN_LOAD_ADC = 0, PGN_LOAD_PA = 1, PGN_LOAD_NORM = 2 } pgn_load_kind;" in header


def test_index_of_bytes_and_strings():
    with P.Pod5File(FIXTURE) as f:
        t = f.reads()
    ids = [bytes(t.read_id[i]) for i in (4, 0, 4, 9)]
    assert t.index_of(ids).tolist() == [4, 0, 4, 9]
    assert t.index_of([str(uuid.UUID(bytes=b)) for b in ids]).tolist() == [4, 0, 4, 9]
    assert t.index_of(t.read_id[[2, 7]]).tolist() == [2, 7]
    assert t.index_of(ids[0]).tolist() == [4] and t.index_of(str(uuid.UUID(bytes=ids[1]))).tolist() == [0]
    assert t.index_of([]).size == 0
    with pytest.raises(KeyError):
        t.index_of([bytes(16)])
    with pytest.raises(KeyError):
        t.index_of(["00000000-0000-0000-0000-000000000001"])


@pytest.mark.parametrize("version,column", [(0, "num_samples"), (1, "num_samples"), (2, "calibration_offset")])
def test_older_layouts_are_refused_by_name(version, column):
    path = os.path.join(REF_DATA, f"multi_fast5_zip_v{version}.pod5")
    if not os.path.exists(path):
        pytest.skip("the reference's test data is not mounted")
    with P.Pod5File(path) as f:
        with pytest.raises(P.Pod5FileError) as e:
            f.reads()
        assert e.value.status == UNSUPPORTED and f"'{column}'" in str(e.value)
        with pytest.raises(P.Pod5FileError) as e2:  # the cached outcome, message included
            f.reads()
        assert e2.value.status == UNSUPPORTED and f"'{column}'" in str(e2.value)


def test_file_without_reads_table_is_unsupported(tmp_path):
    with P.Pod5File(FIXTURE) as f:
        t = f.signal_table()
    p = str(tmp_path / "signal_only.pod5")
    P.write_pod5(p, t, source=None)
    with P.Pod5File(p) as g:
        with pytest.raises(P.Pod5FileError) as e:
            g.reads()
    assert e.value.status == UNSUPPORTED and "no reads table" in str(e.value)


def test_reads_listing_a_missing_row_is_corrupt(tmp_path):
    with P.Pod5File(FIXTURE) as f:
        t = f.signal_table()
        five = P.SignalTable(t.read_ids[:5], t.samples[:5], t.offsets[:6], t.data[:int(t.offsets[5])], t.signal_type)
        p = str(tmp_path / "five_rows.pod5")
        P.write_pod5(p, five, source=f)
    with P.Pod5File(p) as g:
        assert g.rows == 5
        with pytest.raises(P.Pod5FileError) as e:
            g.reads()
    assert e.value.status == CORRUPT and "beyond the table" in str(e.value)


def test_several_read_batches_and_a_keep_going_file(tmp_path):
    from test_pod5_keep_going import _expected, _reads_rows, _rebatched

    src = _rebatched(tmp_path, 3)
    with P.Pod5File(src) as f:
        t = f.reads()
        assert assert_equals_arrow(t, src) == t.batches == 4
        assert lists_of(t) == SIGNAL_LISTS and t.signal_samples.tolist() == SAMPLES
        lists, batches = _reads_rows(src)
        status = np.zeros(22, np.int32)
        status[lists[batches[1][1]][0]] = 9   # batch 1: its second read fails at its first chunk
        status[lists[batches[3][0]][-1]] = 1  # batch 3: its first read fails at its last chunk
        out = str(tmp_path / "kg.pod5")
        P.write_pod5_keep_going(out, f.signal_table(), status, source=f, rows_per_batch=5)
    kept_reads, kept_rows, _ = _expected(lists, batches, status)
    remap = {old: new for new, old in enumerate(kept_rows)}
    with P.Pod5File(out) as g:
        u = g.reads()
        assert_equals_arrow(u, out)
        assert len(u) == len(kept_reads) < 10
        assert lists_of(u) == [[remap[x] for x in SIGNAL_LISTS[r]] for r in kept_reads]
        assert lists_of(u) != [SIGNAL_LISTS[r] for r in kept_reads]  # the rows were renumbered
        assert u.signal_samples.tolist() == [SAMPLES[r] for r in kept_reads]
        assert [bytes(x) for x in u.read_id] == [bytes(t.read_id[r]) for r in kept_reads]
        assert u.calibration_offset.tolist() == [CAL_OFFSET[r] for r in kept_reads]


def test_random_corruptions_give_a_status_or_a_parse(tmp_path):
    raw = open(FIXTURE, "rb").read()
    off, ln = reads_range(FIXTURE)
    rng = np.random.default_rng(20241019)
    p = str(tmp_path / "damaged.pod5")
    outcomes = {}
    for _ in range(300):
        b = bytearray(raw)
        at = off + int(rng.integers(0, ln))
        for k in range(int(rng.integers(1, 5))):
            if at + k < off + ln:
                b[at + k] = int(rng.integers(0, 256))
        open(p, "wb").write(b)
        with P.Pod5File(p) as f:  # the signal table and the file's footer are intact
            try:
                t = f.reads()
                assert t.row_first[0] == 0 and t.row_first[-1] == t.rows.size and (np.diff(t.row_first.astype(np.int64)) >= 0).all()
                assert (t.rows < f.rows).all()
                outcomes[0] = outcomes.get(0, 0) + 1
            except P.Pod5FileError as e:
                assert e.status in (UNSUPPORTED, CORRUPT, _native.PGN_ERR_IO), e
                outcomes[e.status] = outcomes.get(e.status, 0) + 1
    assert sum(outcomes.values()) == 300 and outcomes.get(CORRUPT, 0) + outcomes.get(UNSUPPORTED, 0) > 0


def test_host_sanitizers_on_the_stand_alone_program(tmp_path):
    """tests/c/test_pod5_reads.c with csrc/pgn_pod5file.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer: a program of its own on the CPU (the fixture, copies of it cut short and
    copies with bytes of the reads table overwritten).  The sanitizer runtimes are linked statically, so
    the program does not depend on what else the process environment loads."""
    gxx, gcc = shutil.which("g++"), shutil.which("gcc")
    assert gxx and gcc, "the host compilers build the package; they are needed here too"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    src = os.path.join(ROOT, "rawnanoporesignalcompression_amd", "csrc", "pgn_pod5file.cpp")
    exe = str(tmp_path / "test_pod5_reads")
    for cmd in ([gxx, "-std=c++17", *san, "-c", "-o", str(tmp_path / "pf.o"), src],
                [gcc, "-std=c99", "-Wall", *san, "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"),
                 os.path.join(ROOT, "tests", "c", "test_pod5_reads.c")],
                [gxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-o", exe, str(tmp_path / "t.o"), str(tmp_path / "pf.o")]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cmd, r.stderr)
    r = subprocess.run([exe, FIXTURE, str(tmp_path / "scratch.pod5")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_pod5_reads ok: 10 reads" in r.stdout, (r.returncode, r.stdout, r.stderr[-4000:])
