"""The reads of tests/_select_cases.py check themselves (CPU): every case's predicate -- the property it was
built for -- holds on the sorted read; the statistics the builders state from their histograms are ref_stats'
(np.sort); the set holds every placement the selection's structure distinguishes, on every route; and the host
build of the selection (libpgn_model.so, which compiles walk_ranks, locate, refine, key_mad and rank_of from
csrc/pgn_select.h) equals the reference on every case, field for field.  tests/test_gpu_select_cases.py runs the
same cases through the kernels.
"""
import collections

import numpy as np
import pytest

import _select_cases as S
from test_norm_api import MEDMAD, QUANTILE, assert_stats_equal, model_stats, needs_model, ref_norm, ref_stats

CAT = S.catalogue


def test_every_predicate_holds():
    failed = [c.name for c in CAT() if not c.holds()]
    assert not failed, failed


def test_the_builders_statistics_are_the_references():
    """want comes from a cumulative walk over the histogram the builder laid out (and, for the rank a case is
    about, from the design); ref_stats sorts the samples."""
    for c in CAT():
        r = ref_stats(c.x, **c.prm)
        assert c.want and set(c.want) <= {"q_lo", "q_hi", "m2", "mad4"}, c.name
        assert set(c.want) == ({"q_lo", "q_hi"} if c.prm["mode"] == "quantile" else {"m2", "mad4"}), c.name
        for k, v in c.want.items():
            assert int(r[k]) == v, (c.name, k, int(r[k]), v)


def test_every_family_on_every_route():
    have = collections.defaultdict(set)
    for c in CAT():
        have[c.family].add(c.route)
        assert c.route == S.route_of(c.x.size)
    for family in ("edge", "pair", "round", "mad"):
        assert have[family] == set(S.ROUTES), family
    assert "short" in have["short"] and have["part"] == {"split"}
    # tags that every route must meet
    for tag in ("coarse_edge", "fine_edge", "in_group", "across_groups", "empty_groups", "ends", "both", "lo_last", "lo_first",
                "hi_last", "hi_first", "same_value", "same_bin", "same_group", "other_group", "k_equal", "extremes", "rounding",
                "p_lo", "p_hi", "odd_m2", "key_131070", "max_rank_key", "mad_edge", "mad_zero", "mad_bins", "constant_end",
                "distinct_full"):
        assert {c.route for c in S.tagged(tag)} == set(S.ROUTES), tag
    # every mode at every coarse pair and every fine pair, on every route
    for tag, *_ in S.COARSE_PAIRS:
        for mode in S.MODES:
            assert {c.route for c in S.tagged(tag) if mode in c.tags and "coarse_edge" in c.tags} == set(S.ROUTES), (tag, mode)
    for f1, f2 in S.FINE_PAIRS:
        for mode in S.MODES:
            routes = {c.route for c in S.tagged("fine_edge") if c.name.startswith(f"edge_fine_{f1}_{f2}_{mode}_")}
            assert routes == set(S.ROUTES), (f1, f2, mode)
    assert {(0, 1), (0, 63), (62, 63)} <= set(S.FINE_PAIRS)
    lens = {c.x.size for c in CAT()}
    assert {1, 2, 63, 64, 65, 448, 449, 511, 512, 513, 1023, 1024, 1025} <= lens and max(lens) <= 5000
    # the split reads have 2 to 5 parts
    assert {len(S.parts_of(c.x.size)) - 1 for c in CAT() if c.route == "split"} == {2, 3, 4, 5}


def test_edges_are_where_an_off_by_one_shows():
    """On an edge case the neighbouring rank's sample is another value, so a walk that is one sample off gives
    another statistic; across a coarse edge it is in another bin as well."""
    for c in S.tagged("coarse_edge") + S.tagged("fine_edge"):
        F = S.Facts(c)
        mode = next(m for m in S.MODES if m in c.tags)
        k = F.k[0] if mode.startswith("lo") or mode == "both" else F.k[1]
        other = k + 1 if mode.endswith("last") or mode == "both" else k - 1
        assert F.s[k] != F.s[other], c.name
        if "coarse_edge" in c.tags:
            assert S.pbin(F.s[k]) != S.pbin(F.s[other]), c.name
    ends = S.tagged("ends")
    assert all(c.x.min() == -32768 and c.x.max() == 32767 for c in ends)
    fines = {(S.pfine(S.Facts(c).s[S.Facts(c).k[0]])) for c in S.tagged("fine_edge")}
    assert {0, 63} <= fines


def test_rank_rounding_pairs():
    """The searched (p, n): the binary64 floor differs from the exact floor and from the float32 product's; at
    least two pairs per route; 0.29 at n = 101 is among them (28, where the others give 29)."""
    found = S.search_rounding()
    assert S.three_ranks(29, 101) == (28, 29, 29) and 101 in found[29]
    per_route = collections.Counter()
    for j, ns in found.items():
        for n in ns:
            k64, exact, k32 = S.three_ranks(j, n)
            assert k64 != exact and k64 != k32, (j, n)
            per_route[S.route_of(n)] += 1
    assert all(per_route[r] >= 2 for r in S.ROUTES), per_route
    for c in S.tagged("rounding"):
        which = "q_lo" if "p_lo" in c.tags else "q_hi"
        p = c.prm["p"][0 if "p_lo" in c.tags else 1]
        n = c.x.size
        assert c.want[which] + n // 2 == int(np.floor(np.float64(p) * np.float64(n - 1)))
        assert c.want[which] + n // 2 != int(np.floor(np.float32(p) * np.float32(n - 1)))


def test_mad_key_facts():
    """What the MAD cases claim about keys: 131070 is present and in coarse bin 1023 but the rank's key is at most
    65535 (bin 511); the bin-edge pairs straddle a multiple of 128; every key has m2's parity."""
    for c in S.tagged("key_131070"):
        F = S.Facts(c)
        assert F.keys.max() == 131070 and 131070 >> 7 == 1023 and F.t[F.k[1]] <= 65535, c.name
    assert all(c.want == dict(m2=-1, mad4=131070) for c in S.tagged("max_rank_key"))
    pairs = set()
    for c in S.tagged("mad_edge"):
        F = S.Facts(c)
        assert ((F.keys - F.m2) % 2 == 0).all()
        a, b = int(F.t[F.k[0]]), int(F.t[F.k[1]])
        if a != b:
            pairs.add((a, b))
            assert a >> 7 != b >> 7 and (a & 127 >= 126 and b & 127 <= 1), c.name
    assert pairs == {(127, 129), (126, 128), (255, 257), (254, 256)}
    for c in S.tagged("mad_zero"):
        assert float(ref_stats(c.x, **c.prm)["spread"]) == c.prm["spread_floor"] and c.want["mad4"] == 0
    groups = {(int(S.Facts(c).t[S.Facts(c).k[0]]) >> 9, int(S.Facts(c).t[S.Facts(c).k[1]]) >> 9) for c in S.tagged("mad_bins")}
    assert any(a == b for a, b in groups) and any(a != b for a, b in groups)


def test_split_placement_facts():
    starts = set()
    for c in S.tagged("head_tail"):
        bounds = S.parts_of(c.x.size)
        starts.add((c.phase + bounds[1]) % 8)
        assert c.phase is not None and len(bounds) - 1 >= 2
    assert starts == set(range(8))
    a, b = S.tagged("boundary_pair")
    assert np.array_equal(np.sort(a.x), np.sort(b.x)) and not np.array_equal(a.x, b.x) and a.want == b.want
    bound = S.parts_of(a.x.size)[1]
    assert int(a.x[bound - 1]) == a.want["q_lo"] == int(b.x[bound])
    up, down = [c for c in S.tagged("sorted") if "ascending" in c.name], [c for c in S.tagged("sorted") if "descending" in c.name]
    assert len(up) == len(down) == 2 and np.array_equal(up[0].x, down[0].x[::-1])
    assert {c.prm["mode"] for c in S.tagged("sorted")} == {"quantile", "medmad"}
    # pack() puts a case with a phase where it asks to be
    cases = S.tagged("head_tail") + S.tagged("one_home")
    flat, offsets, counts = S.pack(cases)
    for c, o, n in zip(cases, offsets, counts):
        assert np.array_equal(flat[o:o + n], c.x) and (c.phase is None or o % 8 == c.phase)
    assert (np.diff(offsets) >= counts[:-1]).all()


def test_chain_and_succession():
    """The reads of the many-reads call: the next read's placed bins are the two bins this read fills most, for
    the next read and for the one 1,024 reads on (the read the same workgroup takes next on 256 compute units)."""
    reads = S.chain_reads()
    assert len(reads) >= 1100 and all(513 <= x.size <= 600 for x, _ in reads)

    def heaviest(x):
        bins, cnt = np.unique((x.astype(np.int64) + 32768) >> 6, return_counts=True)
        return set(bins[np.argsort(cnt)[-2:]].tolist())

    checked = 0
    for r, (x, want) in enumerate(reads):
        assert {k: int(v) for k, v in ref_stats(x, **QUANTILE).items() if k in want} == want
        for nxt in (r + 1, r + S.CHAIN_GRID):
            if nxt < len(reads) and S.chain_level(nxt) == S.chain_level(r) + 1:
                w = reads[nxt][1]
                assert {S.pbin(w["q_lo"]), S.pbin(w["q_hi"])} == heaviest(x), (r, nxt)
                checked += 1
    assert checked > 1200
    calls = S.succession()
    split = [sum(x.size > S.SPLIT_MIN for x, _ in rs) for _, rs in calls]
    assert [p["mode"] for p, _ in calls] == ["medmad", "quantile", "medmad"] and split[1] < split[0] < split[2]
    for prm, rs in calls:
        for x, want in rs:
            assert {k: int(v) for k, v in ref_stats(x, **prm).items() if k in want} == want


def test_convert_cases():
    reads, chunks, starts, total = S.convert_reads()
    sizes = {c for cs in chunks for c in cs}
    assert {1, 7, 8, 9, 40} <= sizes and any(2000 < c < 2200 for c in sizes) and all(len(cs) >= 1 for cs in chunks)
    assert (np.diff(starts) > np.array([x.size for x in reads])[:-1]).all() and starts[0] > 0
    assert total > starts[-1] + reads[-1].size
    for dtype, views in S.CONVERT_VIEWS.items():
        for a, b in views:
            assert b is None or S.byte_phase(dtype, a) != S.byte_phase("float16", b), (dtype, a, b)
    assert [a for a, _ in S.CONVERT_VIEWS["float32"]] == [1, 2, 3]
    assert [a for a, b in S.CONVERT_VIEWS["float16"] if b is not None] == list(range(1, 8))
    assert (1, None) in S.CONVERT_VIEWS["float16"]
    # with the destinations a view apart, chunks come out on both sides of the kernel's test: the sample behind
    # the input's head is 16-byte aligned, the output's element there is or is not
    for dtype, views in S.CONVERT_VIEWS.items():
        size = 4 if dtype == "float32" else 2
        for a, b in views:
            if b is None:
                continue
            kinds = set()
            for r, cs in enumerate(chunks):
                at = int(starts[r])
                for c in cs:
                    head = min((-(2 * (b + at)) % 16) // 2, c)
                    if (c - head) >> 3:
                        kinds.add((size * (a + at + head)) % 16 == 0)
                    at += c
            assert False in kinds, (dtype, a, b)


def test_float16_range_parameters():
    """The three parameter sets over all 65,536 values: the usual one stays in the normal range; the large spread
    gives at least 1,000 binary16 subnormals; the floor gives at least 1,000 infinities; and float32 products lie
    exactly on binary16 ties."""
    x = S.all_values_read()
    assert np.array_equal(np.sort(x), np.arange(-32768, 32768))
    ties = {}
    with np.errstate(over="ignore"):
        for key, prm in S.F16_RANGE.items():
            st = ref_stats(x, **prm)
            o32 = ref_norm(x, st["centre"], st["spread"])
            o16 = o32.astype(np.float16)
            sub = int(((np.abs(o16) < np.float16(2.0 ** -14)) & (o16 != 0)).sum())
            inf = int(np.isinf(o16).sum())
            ties[key] = int(S.f16_ties(o32).sum())
            print(key, st["centre"], st["spread"], "subnormal", sub, "infinite", inf, "ties", ties[key])
            if key == "usual":
                assert sub < 100 and inf == 0
            if key == "subnormal":
                assert sub >= 1000
            if key == "overflow":
                assert inf >= 1000 and float(st["spread"]) == prm["spread_floor"]
    assert ties["overflow"] >= 1 and sum(ties.values()) >= 1


@needs_model
def test_host_model_on_every_case():
    for c in CAT():
        assert_stats_equal(model_stats(c.x, **c.prm), ref_stats(c.x, **c.prm), c.name)
    for x, _ in S.chain_reads()[::7]:
        assert_stats_equal(model_stats(x, **QUANTILE), ref_stats(x, **QUANTILE), "chain")
    for prm, rs in S.succession():
        for x, _ in rs:
            assert_stats_equal(model_stats(x, **prm), ref_stats(x, **prm), "succession")
    x = S.all_values_read()
    for prm in list(S.F16_RANGE.values()) + [MEDMAD]:
        assert_stats_equal(model_stats(x, **prm), ref_stats(x, **prm), "all values")
