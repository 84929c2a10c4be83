"""The on-chip search of small single-block frames (csrc/pgn_zenc.h small_search_wave), as its host
model (csrc/zstd1_model.h small_search_serial, model_capi.hip z1m_small_search): a log of committed
writes instead of the hash table, a Bloom filter in front of it.  The model must give what the serial
level-1 search (fast_search_serial) gives -- the same sequences, last literal run and repeat offsets --
on every stream of tests/_small_search_cases.py, and must do so on its own path: the cases that fall
back to the general search are counted, so the test cannot pass by falling back."""
import numpy as np
import pytest

import _oracle as O
import _search_cases as S
import _small_search_cases as SS


def same_search(name, stream):
    a, ia = SS.run(stream, 0)
    b, ib = SS.run(stream, 1)
    assert np.array_equal(a, b), f"{name}: sequences differ"
    for k in ("nbseq", "last_ll", "rep0", "rep1"):
        assert ia[k] == ib[k], f"{name}: {k} {ib[k]}, the serial search {ia[k]}"
    return ib


def test_constants():
    assert SS.small_bytes() >= 1151 and SS.small_bytes() == 2048
    assert len(SS.lengths()) == 12 and len(SS.GENERATORS) == 7


@pytest.mark.parametrize("g", sorted(SS.GENERATORS))
def test_generators(g):
    infos = {n: same_search(n, s) for n, s in SS.generated_cases().items() if n.startswith(g + "/")}
    assert len(infos) == len(SS.lengths())
    # every case ends on the small path but the named ones, whose writes outrun the log
    for n, i in infos.items():
        if n in SS.OVERFLOWING:
            assert i["overflow"] and not i["small"], (n, i)
        else:
            assert i["small"] and not i["overflow"], (n, i)


def test_bench_lhigh_streams():
    infos = [same_search(n, s) for n, s in SS.bench_lhigh().items()]
    assert len(infos) == 50
    for (n, s), i in zip(SS.bench_lhigh().items(), infos):
        a = np.frombuffer(s, np.uint8)
        assert 1000 <= a.size <= SS.small_bytes() and (a == 0).mean() > 0.95, n
        assert i["small"] and not i["overflow"] and i["nbseq"] >= 5, (n, i)
        assert i["log_entries"] <= SS.log_cap() // 2, (n, i)  # far from the log's end
        assert not S.certified(s), n  # the certificate never spares these the search


def test_directed_reach_their_hazards():
    c = SS.directed_cases()
    info = {n: same_search(n, s) for n, s in c.items()}
    assert all(i["small"] and not i["overflow"] for i in info.values()), info
    for lane in S.LANES:
        assert S._lane_count(c[f"lane/{lane}"], lane) >= 2
    i = info["filter/false_positive_then_match"]
    assert i["refuted_absent"] >= 1 and i["fp_then_hit"] >= 1, i
    i = info["filter/shadowed"]
    assert i["shadowed"] >= 1 and SS.no_match_at_shadow(c["filter/shadowed"]), i
    assert (S.profile(c["repcode/after_match"])[:, S.KIND] == S.POST_REP).sum() >= 3
    assert len(S.anchor_stopped_rows(c["back/anchor_stop"])) > 0
    for g in SS.END_GAPS:
        assert SS.ends_at(c[f"end/gap{g}"], g), g


def test_bound_cases_run_the_exact_search_to_the_blocks_end():
    """Streams of kSmallSearchBytes - 1 and kSmallSearchBytes bytes that the certificate does not spare and
    the small search finishes: long runs (matches and log entries up to the last positions), and a match
    that ends at the block's last byte and 1 .. 8 bytes before it."""
    c = SS.bound_cases()
    assert len(c) == 2 * (3 + len(SS.END_GAPS))
    for n, s in c.items():
        i = same_search(n, s)
        assert len(s) in SS.bound_sizes() and not S.certified(s), n
        assert i["small"] and not i["overflow"], (n, i)
        rows = S.profile(s)
        assert rows[-1][S.POS] > len(s) - 200, (n, rows[-1])  # sequences up to the block's end
        if n.startswith("bound_runs/"):
            a = np.frombuffer(s, np.uint8)
            assert (a == 0).mean() > 0.9 and i["nbseq"] >= 20 and i["rep_first"] >= 10, (n, i)
        else:
            assert SS.ends_at(s, int(n.rsplit("gap", 1)[1])), n


def test_overflow_and_beyond_fall_back():
    i = same_search("overflow", SS.overflow_case())
    assert i["overflow"] == 1 and i["small"] == 0 and len(SS.overflow_case()) <= SS.small_bytes()
    s = SS.beyond_case()
    assert len(s) == SS.small_bytes() + 1
    i = same_search("beyond", s)
    assert i["small"] == 0 and i["overflow"] == 0 and i["nbseq"] > 0


def test_path_counts():
    """Every case ends on the small path except the one too large and those whose log overflows: the
    overflow stream and the named generated cases (matchy or noise-like blocks of 1,151 bytes and more
    that fail the certificate), no other."""
    info = {n: same_search(n, s) for n, s in SS.cases().items()}
    over = sorted(n for n, i in info.items() if i["overflow"])
    small = sorted(n for n, i in info.items() if i["small"])
    assert over == sorted(SS.OVERFLOWING + ("overflow/small_alphabet",)), over
    assert sorted(set(info) - set(small)) == sorted(over + ["beyond/runs"])
    assert len(info) == 7 * 12 + 50 + 16 + 24 + 2 and len(small) == len(info) - 15
    # the searches did work: rounds, log entries and filter hits all occur in the set
    assert sum(i["rounds"] for i in info.values()) > 1000  # the bench streams alone: 50 of 12 rounds or more
    assert sum(i["scans"] for i in info.values()) > 200
    assert sum(i["refuted"] for i in info.values()) > 20


def test_streams_are_the_chunks_lhigh_streams():
    for name, (x, blob) in SS.reference().items():
        st = O.c5_streams(x)
        assert st[4] == SS.cases()[name] and len(st[1]) == 0 and len(st[2]) == 0 and len(st[3]) == x.size, name
