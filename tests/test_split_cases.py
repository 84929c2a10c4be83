"""The catalogue of tests/_split_cases.py on the CPU: every claim of every case holds in the shape model, the
restatement in the device's shape gives the oracle's streams, the oracle's streams are the reference's own
(where the reference tree is present), every named fault of the restatement changes the streams of some case
for every codec it exists in, and every case compresses with status 0 at the reference's capacity under all
seven codecs, so that no GPU route has to skip one.  tests/test_gpu_split_cases.py runs the same cases
through every route that reaches a split kernel."""
import numpy as np
import pytest

import _oracle as O
import _split_cases as S
from test_oracle_ref import needs_ref

MAX_CASES, MAX_SAMPLES = 210, 3_000_000  # what keeps the GPU tests at seconds
FAULT_MAX_N = 70000                      # the faults are looked for on the cases up to this size


def test_catalogue_size_and_families():
    cat = S.catalogue()
    total = sum(c.n for c in cat)
    print(f"{len(cat)} cases, {total} samples")
    assert len(cat) <= MAX_CASES and total <= MAX_SAMPLES
    assert len(cat) == 204 and total == 2581256
    assert {c.family for c in cat} == set(S.FAMILIES)
    assert all(set(c.codecs) <= set(S.CODECS) and c.claims for c in cat if c.family != "values" or c.claims)
    per = {f: len(S.cases(family=f)) for f in S.FAMILIES}
    assert per == {"values": 5, "seams": 4, "counts": 72, "carries": 46, "ragged": 57, "ranges": 16, "capacity": 4}
    ragged = sorted(c.n for c in S.cases(family="ragged"))
    assert ragged == sorted(1024 * k + r for k in (0, 1, 2) for r in S.RAGGED_R)
    assert {n % 8 for n in ragged} == set(range(8))
    for codec in S.CODECS:  # every codec has cases of every family meant for it
        assert {c.family for c in S.cases(codec=codec)} == set(S.FAMILIES), codec
    assert sorted(c.n for c in S.cases(family="capacity")) == [262144] * 3 + [262144 + 1031]


def test_range_plan_is_the_kernels():
    for steps, held in ((1, 1), (2, 2), (31, 31), (32, 32), (33, 32), (47, 32), (64, 32), (256, 32)):
        plan = S.range_plan(steps * 1024 - 24)
        assert plan[0][0] == 0 and plan[-1][1] == steps * 1024 - 24
        assert all(a[1] == b[0] or a[0] >= a[1] for a, b in zip(plan, plan[1:]) if b[0] < b[1])
        assert sum(t0 < t1 for t0, t1 in plan) == held
        assert [t0 for t0, _ in plan] == [1024 * (steps * r // 32) for r in range(32)]


def test_every_claim_holds_in_the_shape_model():
    wrong, count = [], 0
    for c in S.catalogue():
        shapes = {}
        for text, (codec, holds) in c.claims.items():
            if codec not in shapes:
                shapes[codec] = S.split_shape(c.x, codec)
            count += 1
            if not holds(shapes[codec]):
                wrong.append(f"{c.name}: {text}")
    print(f"{count} claims")
    assert count >= 350
    assert not wrong, wrong


def test_shape_model_counts_are_the_streams():
    """the model's totals are the oracle's stream lengths: it is not a second opinion on the classes"""
    for c in S.catalogue()[::9]:
        sh = S.split_shape(c.x, "C5")
        st = O.c5_streams(c.x)
        assert [len(s) for s in st] == [(c.n + 3) // 4, (sh["totals"][0] + 1) // 2, sh["totals"][1], sh["totals"][2],
                                        sh["totals"][2]], c.name
        assert sum(g["cS"] for g in sh["ranges"]) == sh["totals"][0]
        assert sum(s["S"]["blocks"] for s in sh["steps"]) * 16 + (sh["steps"][-1]["S"]["after"] + 1) // 2 == len(st[1])


@pytest.mark.parametrize("codec", S.CODECS)
def test_restatement_equals_the_oracle(codec):
    """without a fault, by the one-wave walk and (C5) by the 32 ranges"""
    wrong = []
    for c in S.catalogue():
        want = S.oracle_streams(c.x, codec)
        routes = [False, True] if codec == "C5" and c.n <= S.PASS_SAMPLES else [False]
        for ranges in routes:
            got = S.split_as_device(c.x, codec, ranges=ranges)
            if got != want:
                wrong.append((c.name, "ranges" if ranges else "wave", [i for i, (g, w) in enumerate(zip(got, want)) if g != w]))
    assert not wrong, wrong[:10]


@needs_ref
@pytest.mark.parametrize("codec", S.CODECS)
def test_oracle_equals_the_reference(codec):
    """the catalogue pins the oracle too: the streams of the reference's own compiled encoders"""
    for c in S.catalogue():
        assert S.oracle_streams(c.x, codec) == S.ref_streams(c.x, codec), c.name


def _tells(fault, codec, cat, want):
    routes = [True] if fault in S.RANGE_FAULTS else ([False, True] if codec == "C5" else [False])
    for c in cat:
        if codec not in c.codecs:
            continue
        if (c.name, codec) not in want:
            want[c.name, codec] = S.oracle_streams(c.x, codec)
        for ranges in routes:
            try:
                got = S.split_as_device(c.x, codec, ranges=ranges, fault=fault)
            except (AssertionError, IndexError, ValueError):
                got = None  # the fault walked out of a window: told as well
            if got != want[c.name, codec]:
                return f"{c.name} ({'ranges' if ranges else 'wave'})"
    return None


def test_every_fault_is_told_by_a_case():
    """fault -> the first case whose streams it changes, for every codec the fault exists in.  A fault that no
    case tells is a missing case."""
    cat = S.cases(max_n=FAULT_MAX_N)
    want, table = {}, {}
    for fault, codecs in S.FAULTS.items():
        for codec in codecs:
            table[fault, codec] = _tells(fault, codec, cat, want)
    print()
    for (fault, codec), hit in table.items():
        print(f"{fault:18s} {codec:5s} {hit}")
    assert len(S.FAULTS) == 14
    assert not [k for k, hit in table.items() if hit is None]
    for fault in ("lane0_prev", "tail_keys"):
        assert set(S.FAULTS[fault]) == set(S.CODECS)
    for fault in ("carry_dropped", "odd_nibble_high"):
        assert {"VBZ0"} <= set(S.FAULTS[fault])


def test_faults_are_told_by_the_cases_built_for_them():
    """beyond the first teller: the case a hazard was built into tells its fault"""
    built = {
        "field3_wrap": ("counts/class3_in_0_x1024", "C5", False),
        "full_window_63": ("counts/class2_in_0_x1024", "C5", False),
        "carry_dropped": ("carries/starved_class2", "C5", False),
        "empty_range_owner": ("ranges/no_class1_between_odd_neighbours_32_steps", "C5", True),
        "last_half_owner": ("ranges/no_class1_in_the_last_ranges_33_steps", "C5", True),
        "late_first_entry": ("ranges/first_entry_in_the_second_step_64_steps", "C5", True),
        "lead_written": ("ranges/starts_inside_a_block_0", "C5", True),
        "odd_lead_byte": ("ranges/starts_inside_a_block_1", "C5", True),
        "range_prev": ("seams/ranges_33_large_among_small", "C5", True),
        "lane0_prev": ("seams/small_among_large_3112", "VBZ", False),
        "half_borrow": ("values/borrow_pairs_1024", "C4", False),
        "threshold_ge": ("values/thresholds_1024_first_zero", "C4", False),
        "tail_keys": ("ragged/1x1024_plus_5", "C5", False),
        "odd_nibble_high": ("values/int16_wrap_1040", "VBZ0", False),
    }
    assert set(built) == set(S.FAULTS)
    by_name = {c.name: c for c in S.catalogue()}
    for fault, (name, codec, ranges) in built.items():
        c = by_name[name]
        try:
            got = S.split_as_device(c.x, codec, ranges=ranges, fault=fault)
        except (AssertionError, IndexError, ValueError):
            got = None
        assert got != S.oracle_streams(c.x, codec), (fault, name)


@pytest.mark.parametrize("codec", S.CODECS)
def test_every_case_fits_the_reference_capacity(codec):
    """status 0 at the reference's own capacity, so the per-chunk route runs every case"""
    worst = 0.0
    for c in S.catalogue():
        if codec == "VBZ":
            blob = O.vbz_compress(c.x)  # asserts status 0 at the reference's VBZ bound
            size, cap = len(blob), int(O.oracle().pgno_vbz_bound(c.n))
        else:
            rc, blob, _ = (O.c5_compress(c.x) if codec == "C5" else O.variant_compress(codec, c.x))
            assert rc == O.OK, (c.name, rc)
            size, cap = len(blob), int(O.oracle().pgno_c5_bound(c.n))
        assert size <= cap, c.name
        worst = max(worst, size / cap)
    print(f"{codec}: largest blob / capacity {worst:.3f}")


def test_restatement_round_trip():
    """the restatement's streams decode to the samples (the oracle's merge over them)"""
    for c in S.catalogue()[::17]:
        st = S.split_as_device(c.x, "C5", ranges=c.n <= S.PASS_SAMPLES)
        rc, back, _ = O.oracle_variant_merge("C5", b"".join(st), [len(s) for s in st], c.n)
        assert rc == 0 and np.array_equal(back, c.x), c.name
