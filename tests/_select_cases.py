"""Reads built for the bins and ranks of the per-read selection (tests only, CPU only, numpy).

csrc/pgn_select.h selects exactly, by radix: a key's top 10 bits give one of 1,024 coarse bins (summed in groups
of four for a two-level rank walk), the key's low bits a fine histogram per rank.  What decides whether a wrong
walk, key or rank formula shows is where the ranks fall among the bins, so the reads here are laid out from a
histogram -- a sorted list of (value, count) -- after the rank is chosen: k = floor(float64(p) * float64(n - 1))
first, then counts so that the k-th sorted sample is where the case wants it.  A read is shuffled with a pinned
seed unless the case is about order.

  plain key = x + 32768; coarse bin = key >> 6; group = bin >> 2; fine = key & 63
  MAD key   = |2x - m2|; coarse bin = key >> 7; fine = key & 127  (every key has the parity of m2)

catalogue() gives Case objects that unpack as (name, read int16, parameter dict, predicate).  A case carries
`want`, the statistics its builder intends (q_lo and q_hi, or m2 and mad4), stated from the histogram by a
cumulative walk and, for the rank the case is about, by the design itself; `pred`, the property it exists for,
a function of Facts (the sorted read, the ranks, the keys); `route` ("short": n <= 512, one wave; "wg": up to
1,024, one workgroup; "split": above, selected in parts under set_select_split(1024, 1024, ...)); and, where the
part a sample lies in matters, `phase`: the read's first element must lie at that offset modulo 8 from a
16-byte boundary (pack() honours it).

Families: edge (a rank on a coarse or fine bin edge), pair (how the two ranks' bins relate), round (p and n for
which the binary64 product's floor is neither the exact one nor float32's), mad (MAD keys), short (the one-wave
kernel's ends), part (what a part of a split read holds and where the rank's sample lies in it).  chain_reads()
and succession() build the reads of the calls in succession; CONVERT_* and F16_RANGE the convert pass's cases.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from test_norm_api import MEDMAD, QUANTILE

SEED = 20261020
SHORT_MAX, SPLIT_MIN, PART = 512, 1024, 1024
SHORT_NS = (63, 64, 65, 448, 449, 511, 512)
WG_NS = (513, 800, 1023, 1024)
SPLIT_NS = (1025, 2049, 3000, 4000, 5000)
ROUTES = ("short", "wg", "split")
P_EQUAL = dict(QUANTILE, p=(0.5, 0.5))
EXTREMES = dict(QUANTILE, p=(0.0, 1.0))


def rank(p, n):
    return int(np.floor(np.float64(p) * np.float64(n - 1)))


def route_of(n):
    return "short" if n <= SHORT_MAX else ("wg" if n <= SPLIT_MIN else "split")


def val(b, f):
    """The sample in plain coarse bin b with fine value f."""
    assert 0 <= b < 1024 and 0 <= f < 64
    return ((b << 6) | f) - 32768


def pbin(v):
    return (int(v) + 32768) >> 6


def pfine(v):
    return (int(v) + 32768) & 63


def parts_of(n):
    """The part boundaries of a read of n samples under the tests' split settings (host.select_parts)."""
    from rawnanoporesignalcompression_amd import select_parts

    return [int(b) for b in select_parts(n, SPLIT_MIN, PART)]


# ---- histograms ---------------------------------------------------------------------------------------------
def norm_hist(hist):
    """Sorted by value, equal values merged, empty entries dropped."""
    acc = {}
    for v, c in hist:
        assert c >= 0 and -32768 <= v <= 32767, (v, c)
        if c:
            acc[int(v)] = acc.get(int(v), 0) + int(c)
    return sorted(acc.items())


def hist_at(hist, k):
    """The value of rank k of a (key, count) list, by a cumulative walk (no sort of samples)."""
    cum = 0
    for v, c in sorted(hist):
        if k < cum + c:
            return v
        cum += c
    raise AssertionError("rank beyond the histogram")


def mad_hist(hist, m2):
    acc = {}
    for v, c in hist:
        key = abs(2 * v - m2)
        acc[key] = acc.get(key, 0) + c
    return sorted(acc.items())


def lay(hist, seed, shuffle=True):
    h = norm_hist(hist)
    x = np.repeat(np.array([v for v, _ in h], np.int64), np.array([c for _, c in h], np.int64))
    if shuffle:
        x = np.random.default_rng(seed).permutation(x)
    return x.astype(np.int16)


def share(count, values):
    """count samples over the values, as evenly as it goes (the first values take the remainder)."""
    if count <= 0:
        return []
    q, r = divmod(count, len(values))
    return [(v, q + (1 if i < r else 0)) for i, v in enumerate(values)]


# ---- cases --------------------------------------------------------------------------------------------------
class Facts:
    """What a predicate may look at: the sorted read, the ranks and the keys, all from np.sort."""

    def __init__(self, case):
        x = case.x.astype(np.int64)
        self.x, self.n, self.s = x, x.size, np.sort(x)
        n = self.n
        if case.prm["mode"] == "quantile":
            self.k = (rank(case.prm["p"][0], n), rank(case.prm["p"][1], n))
        else:
            self.k = ((n - 1) // 2, n // 2)
        self.m2 = int(self.s[(n - 1) // 2] + self.s[n // 2])
        self.keys = np.abs(2 * x - self.m2)
        self.t = np.sort(self.keys)

    def bins(self, i):
        """(coarse bin, fine) of the sorted sample i."""
        return pbin(self.s[i]), pfine(self.s[i])


class Case:
    def __init__(self, name, family, x, prm, want, pred, phase=None, tags=()):
        self.name, self.family = name, family
        self.x = np.ascontiguousarray(x, np.int16)
        self.x.setflags(write=False)
        self.prm, self.want, self.pred, self.phase = dict(prm), dict(want), pred, phase
        self.tags = set(tags)
        self.route = route_of(self.x.size)

    def __iter__(self):  # (name, read, parameters, predicate)
        return iter((self.name, self.x, self.prm, self.pred))

    def __repr__(self):
        return f"Case({self.name}, n {self.x.size})"

    def holds(self):
        return bool(self.pred(Facts(self)))


def want_of(hist, prm):
    """The intended statistics, from the histogram alone."""
    h = norm_hist(hist)
    n = sum(c for _, c in h)
    if prm["mode"] == "quantile":
        return dict(q_lo=hist_at(h, rank(prm["p"][0], n)), q_hi=hist_at(h, rank(prm["p"][1], n)))
    m2 = hist_at(h, (n - 1) // 2) + hist_at(h, n // 2)
    t = mad_hist(h, m2)
    return dict(m2=m2, mad4=hist_at(t, (n - 1) // 2) + hist_at(t, n // 2))


def from_hist(name, family, hist, prm, pred, designed=None, seed=0, tags=(), x=None, phase=None):
    """A case over a histogram; `designed` are the values the design itself names, checked against the walk."""
    want = want_of(hist, prm)
    for k, v in (designed or {}).items():
        assert want[k] == v, (name, k, want[k], v)
    if x is None:
        x = lay(hist, SEED + seed)
    else:  # an order of the case's own: the same samples
        assert np.array_equal(np.sort(np.asarray(x, np.int64)), lay(hist, 0, shuffle=False).astype(np.int64)), name
    return Case(name, family, x, prm, want, pred, phase, tags)


def both_params(n, p_lo=0.3):
    """Quantile parameters whose two ranks are neighbours: (kLo, kLo + 1)."""
    k = rank(p_lo, n)
    p_hi = (k + 1.5) / (n - 1)
    assert rank(p_hi, n) == k + 1 and p_hi <= 1.0
    return dict(QUANTILE, p=(p_lo, p_hi))


def lengths(i, both=False):
    """One length per route for the i-th case of a family (fixed lengths where the parameters depend on n)."""
    if both:
        return (300, 800, 2500)
    return (SHORT_NS[i % len(SHORT_NS)], WG_NS[i % len(WG_NS)], SPLIT_NS[i % len(SPLIT_NS)])


MODES = ("lo_last", "lo_first", "hi_last", "hi_first", "both")


def boundary(mode, prm, n):
    """(samples below the edge, the rank the mode is about, whether it is the last below or the first above)."""
    kLo, kHi = rank(prm["p"][0], n), rank(prm["p"][1], n)
    k = kLo if mode.startswith("lo") or mode == "both" else kHi
    last = mode.endswith("last") or mode == "both"
    return (k + 1 if last else k), k, last


# ---- family 1: a rank on an edge of the walk -----------------------------------------------------------------
COARSE_PAIRS = [  # (tag, b1, b2, filler bin below or None)
    ("in_group", 4 * 37 + 1, 4 * 37 + 2, 3),
    ("in_group_high", 4 * 200 + 1, 4 * 200 + 2, 4 * 199 + 3),
    ("across_groups", 4 * 100 + 3, 4 * 101, 3),
    ("across_groups_low", 3, 4, None),
    ("empty_groups", 4 * 50 + 2, 4 * 57 + 1, 4 * 40),
    ("ends", 0, 1023, None),
]
TOP_FINE, BOTTOM_FINE = 41, 22  # the unique last sample of b1 and the unique first sample of b2


def coarse_edge_pred(tag, mode, b1, b2):
    def pred(F):
        kLo, kHi = F.k
        k = kLo if mode.startswith("lo") or mode == "both" else kHi
        if mode.endswith("last") or mode == "both":
            ok = F.bins(k) == (b1, TOP_FINE) and F.bins(k + 1) == (b2, BOTTOM_FINE) and F.bins(k - 1)[1] < TOP_FINE
        else:
            ok = F.bins(k) == (b2, BOTTOM_FINE) and F.bins(k - 1) == (b1, TOP_FINE) and F.bins(k + 1)[1] > BOTTOM_FINE
        if mode == "both":
            ok = ok and kHi == kLo + 1 and F.bins(kHi) == (b2, BOTTOM_FINE)
        between = ((F.s + 32768) >> 6 > b1) & ((F.s + 32768) >> 6 < b2)
        ok = ok and not between.any()
        if tag.startswith("in_group"):
            ok = ok and b1 >> 2 == b2 >> 2
        elif tag.startswith("across_groups"):
            ok = ok and b2 == b1 + 1 and b2 >> 2 == (b1 >> 2) + 1
        elif tag == "empty_groups":
            ok = ok and (b2 >> 2) - (b1 >> 2) - 1 >= 5
        else:
            ok = ok and (b1, b2) == (0, 1023) and F.s[0] == -32768 and F.s[-1] == 32767
        return ok

    return pred


def _edge_coarse(out):
    i = 0
    for tag, b1, b2, filler in COARSE_PAIRS:
        for mode in MODES:
            for n in lengths(i, mode == "both"):
                prm = both_params(n) if mode == "both" else dict(QUANTILE)
                below, k, last = boundary(mode, prm, n)
                c0 = n // 10 if filler is not None else 0
                c1, c2 = below - c0, n - below
                assert c1 >= 2 and c2 >= 2, (tag, mode, n)
                hist = share(c0, [val(filler, 5), val(filler, 50)]) if c0 else []
                hist += [(val(b1, TOP_FINE), 1)] + share(c1 - 1, [val(b1, 0), val(b1, 7), val(b1, TOP_FINE - 1)])
                hist += [(val(b2, BOTTOM_FINE), 1)] + share(c2 - 1, [val(b2, 63), val(b2, 50), val(b2, BOTTOM_FINE + 1)])
                q = val(b1, TOP_FINE) if last else val(b2, BOTTOM_FINE)
                designed = {"q_lo" if (mode.startswith("lo") or mode == "both") else "q_hi": q}
                if mode == "both":
                    designed["q_hi"] = val(b2, BOTTOM_FINE)
                out.append(from_hist(f"edge_coarse_{tag}_{mode}_n{n}", "edge", hist, prm, coarse_edge_pred(tag, mode, b1, b2),
                                     designed, seed=i, tags={"coarse_edge", tag, mode}))
            i += 1


FINE_PAIRS = [(0, 1), (0, 63), (31, 32), (62, 63), (5, 40)]


def fine_edge_pred(mode, b, f1, f2):
    def pred(F):
        kLo, kHi = F.k
        k = kLo if mode.startswith("lo") or mode == "both" else kHi
        if mode.endswith("last") or mode == "both":
            ok = F.bins(k) == (b, f1) and F.bins(k + 1) == (b, f2)
        else:
            ok = F.bins(k) == (b, f2) and F.bins(k - 1) == (b, f1)
        if mode == "both":
            ok = ok and kHi == kLo + 1
        inside = F.s[((F.s + 32768) >> 6) == b]
        return ok and set(((inside + 32768) & 63).tolist()) == {f1, f2}

    return pred


def _edge_fine(out):
    i = 0
    for f1, f2 in FINE_PAIRS:
        for mode in MODES:
            b = (4 * 60 + 1, 4 * 120, 4 * 9 + 3)[i % 3]
            for n in lengths(i, mode == "both"):
                prm = both_params(n) if mode == "both" else dict(QUANTILE)
                below, k, last = boundary(mode, prm, n)
                c0, c3 = n // 10, n // 20
                c1 = below - c0
                c2 = n - below - c3
                assert c1 >= 1 and c2 >= 1, (f1, f2, mode, n)
                hist = share(c0, [val(b - 9, 3), val(b - 9, 30)]) + [(val(b, f1), c1), (val(b, f2), c2)]
                hist += share(c3, [val(b + 6, 1), val(b + 6, 63)])
                designed = {"q_lo" if (mode.startswith("lo") or mode == "both") else "q_hi": val(b, f1 if last else f2)}
                if mode == "both":
                    designed["q_hi"] = val(b, f2)
                out.append(from_hist(f"edge_fine_{f1}_{f2}_{mode}_n{n}", "edge", hist, prm, fine_edge_pred(mode, b, f1, f2),
                                     designed, seed=100 + i, tags={"fine_edge", mode}))
            i += 1


# ---- family 2: how the two ranks relate ----------------------------------------------------------------------
def _pair(out):
    g = 77
    lo_bin, hi_bin = 4 * g + 1, 4 * g + 2
    far_bin = 4 * (g + 30) + 2
    for i in range(2):
        for n in lengths(i + 2):
            a, b = n // 20, n // 2
            # one value under both ranks, other fine values of its bin on both sides
            v = val(lo_bin, 33)
            hist = share(a, [val(lo_bin, 2), val(lo_bin, 32)]) + [(v, n - 2 * a)] + share(a, [val(lo_bin, 34), val(lo_bin, 63)])
            out.append(from_hist(f"pair_same_value_n{n}", "pair", hist, QUANTILE,
                                 lambda F: F.k[0] != F.k[1] and F.s[F.k[0]] == F.s[F.k[1]] and F.s[0] < F.s[F.k[0]] < F.s[-1]
                                 and pbin(F.s[0]) == pbin(F.s[-1]), dict(q_lo=v, q_hi=v), seed=200 + i, tags={"same_value"}))
            # one coarse bin, two fine values, fillers in other bins
            hist = [(val(lo_bin - 5, 9), a), (val(lo_bin, 11), b - a), (val(lo_bin, 52), n - b - a), (val(lo_bin + 9, 60), a)]
            out.append(from_hist(f"pair_same_bin_n{n}", "pair", hist, QUANTILE,
                                 lambda F: F.bins(F.k[0])[0] == F.bins(F.k[1])[0] and F.bins(F.k[0])[1] != F.bins(F.k[1])[1],
                                 dict(q_lo=val(lo_bin, 11), q_hi=val(lo_bin, 52)), seed=210 + i, tags={"same_bin"}))
            # neighbouring bins of one group, and bins of different groups; the two bins' fine values differ
            for tag, hb in (("same_group", hi_bin), ("other_group", far_bin)):
                hist = share(b, [val(lo_bin, 4), val(lo_bin, 19), val(lo_bin, 44)]) + share(n - b, [val(hb, 12), val(hb, 27), val(hb, 58)])

                def pred(F, tag=tag):
                    (b0, _), (b1, _) = F.bins(F.k[0]), F.bins(F.k[1])
                    return b0 != b1 and ((b0 >> 2 == b1 >> 2) if tag == "same_group" else (b0 >> 2 != b1 >> 2))

                out.append(from_hist(f"pair_{tag}_n{n}", "pair", hist, QUANTILE, pred, seed=220 + i, tags={tag}))
            # p_lo == p_hi: one rank, asked for twice
            hist = share(n, [val(lo_bin, 8), val(lo_bin, 9), val(hi_bin, 0), val(far_bin, 63), val(far_bin + 1, 0)])
            out.append(from_hist(f"pair_k_equal_n{n}", "pair", hist, P_EQUAL, lambda F: F.k[0] == F.k[1], seed=230 + i,
                                 tags={"k_equal"}))
            # p = (0, 1): minimum and maximum, in one coarse bin and in bins 0 and 1023
            hist = [(val(lo_bin, 3), 1), (val(lo_bin, 60), 1)] + share(n - 2, [val(lo_bin, 4), val(lo_bin, 30), val(lo_bin, 59)])
            out.append(from_hist(f"pair_extremes_one_bin_n{n}", "pair", hist, EXTREMES,
                                 lambda F: F.k == (0, F.n - 1) and pbin(F.s[0]) == pbin(F.s[-1]) and F.s[0] < F.s[1]
                                 and F.s[-2] < F.s[-1], dict(q_lo=val(lo_bin, 3), q_hi=val(lo_bin, 60)), seed=240 + i,
                                 tags={"extremes"}))
            hist = [(-32768, 1), (32767, 1)] + share(n - 2, [-32767, val(lo_bin, 30), 32766])
            out.append(from_hist(f"pair_extremes_ends_n{n}", "pair", hist, EXTREMES,
                                 lambda F: F.k == (0, F.n - 1) and (pbin(F.s[0]), pbin(F.s[-1])) == (0, 1023) and F.s[0] < F.s[1]
                                 and F.s[-2] < F.s[-1], dict(q_lo=-32768, q_hi=32767), seed=250 + i, tags={"extremes"}))
    for n, vals in ((1, [val(far_bin, 63)]), (2, [val(far_bin + 1, 0), val(far_bin, 63)])):  # n = 2: neighbouring values in neighbouring bins
        out.append(from_hist(f"pair_k_equal_n{n}", "pair", [(v, 1) for v in vals], P_EQUAL, lambda F: F.k == (0, 0),
                             dict(q_lo=min(vals), q_hi=min(vals)), tags={"k_equal"}))


# ---- family 3: the rank formula's rounding -------------------------------------------------------------------
def three_ranks(j, n):
    """floor(p (n - 1)) for p = j / 100: (binary64 product, exact rational, float32 product)."""
    p = j / 100
    k32 = int(np.floor(np.float32(p) * np.float32(n - 1)))
    exact = int(Fraction(j, 100) * (n - 1))
    return rank(p, n), exact, k32


def search_rounding(per_route=2, ps=2):
    """{p: [n, ...]}: the first `ps` multiples of 0.01 that have, on every route, lengths at which the binary64
    floor differs from both the exact floor and the float32 product's; `per_route` lengths per route."""
    found = {}
    for j in range(1, 100):
        hits = {r: [] for r in ROUTES}
        for n in range(2, SPLIT_NS[-1] + 1):
            k64, exact, k32 = three_ranks(j, n)
            if k64 != exact and k64 != k32 and len(hits[route_of(n)]) < per_route:
                hits[route_of(n)].append(n)
        if all(hits[r] for r in ROUTES):
            found[j] = [n for r in ROUTES for n in hits[r]]
            if len(found) == ps:
                break
    assert len(found) == ps, found
    return found


def _round(out):
    for j, ns in search_rounding().items():
        p = j / 100
        for n in ns:
            k64, exact, k32 = three_ranks(j, n)
            assert k64 != exact and k64 != k32
            c = n // 2
            hist = [(i - c, 1) for i in range(n)]  # a ramp: the statistic names its rank
            for use, prm in (("p_lo", dict(QUANTILE, p=(p, 0.97))), ("p_hi", dict(QUANTILE, p=(0.03, p)))):
                which = 0 if use == "p_lo" else 1

                def pred(F, which=which, k64=k64, exact=exact, k32=k32, c=c):
                    got = int(F.s[F.k[which]]) + c
                    return got == k64 and got != exact and got != k32 and (np.diff(F.s) == 1).all()

                out.append(from_hist(f"round_{j}_{use}_n{n}", "round", hist, prm, pred,
                                     {"q_lo" if use == "p_lo" else "q_hi": k64 - c}, seed=300 + n, tags={"rounding", use}))


# ---- family 4: med/MAD -----------------------------------------------------------------------------------------
def mad_symmetric(m2, key_hist):
    """A value histogram whose twice-median is m2 and whose MAD keys are key_hist = [(key, even count)]: half of
    every key's samples lie below m2 / 2 and half above (key 0: all at m2 / 2)."""
    hist = []
    for key, cnt in key_hist:
        assert cnt % 2 == 0 and (key - m2) % 2 == 0 and key >= 0
        if key == 0:
            hist.append((m2 // 2, cnt))
        else:
            hist += [((m2 - key) // 2, cnt // 2), ((m2 + key) // 2, cnt // 2)]
    return hist


def mad_lengths(i):
    """Multiples of four (the symmetric layout needs n / 2 even), one per route."""
    return ((300, 448, 512)[i % 3], (516, 800, 1024)[i % 3], (1028, 2400, 4100)[i % 3])


def _mad(out):
    i = 0
    # odd m2: every key odd
    for d in (1, 3):
        for n in mad_lengths(i):
            a = 407
            hist = share(n // 2, [a - 20, a - 3, a]) + share(n // 2, [a + d, a + d + 6, a + d + 30])
            out.append(from_hist(f"mad_odd_m2_d{d}_n{n}", "mad", hist, MEDMAD,
                                 lambda F: F.n % 2 == 0 and F.m2 % 2 == 1 and (F.keys % 2 == 1).all(), dict(m2=2 * a + d),
                                 seed=400 + i, tags={"odd_m2"}))
        i += 1
    # odd m2 with both middle keys from samples below the median: the layouts above and below are symmetric about
    # the median, where a key that is one off towards the median on one side is one off away from it on the other
    # and mad4 does not move
    for n in mad_lengths(i):
        a = -1203
        hist = [(a - 3, n // 2 - 1), (a, 1), (a + 1, 1), (a + 2, n // 4), (a + 1000, n // 2 - 1 - n // 4)]
        out.append(from_hist(f"mad_odd_m2_one_side_n{n}", "mad", hist, MEDMAD,
                             lambda F, a=a: F.m2 == 2 * a + 1 and F.t[F.k[0]] == F.t[F.k[1]] == 7 and (F.keys[F.x > a] != 7).all(),
                             dict(m2=2 * a + 1, mad4=14), seed=405 + i, tags={"odd_m2", "one_side"}))
    i += 1
    # the median at one end of int16, a minority at the other: key 131070 is counted and is never the rank
    for tag, med, other in (("min", -32768, 32767), ("max", 32767, -32768)):
        for n in lengths(i):
            minority = (3 * n) // 10
            out.append(from_hist(f"mad_median_{tag}_n{n}", "mad", [(med, n - minority), (other, minority)], MEDMAD,
                                 lambda F: (F.keys == 131070).any() and (F.keys.max() >> 7) == 1023 and F.t[F.k[1]] == 0,
                                 dict(m2=2 * med, mad4=0), seed=410 + i, tags={"key_131070"}))
        i += 1
        # odd n with exactly (n + 1) / 2 samples at the median: the MAD rank is the last key 0
        for n in (449, 801, 2049):
            rest = (n - 1) // 2
            hist = [(med, n - rest), (other, rest - 1), (med + (1 if tag == "min" else -1), 1)]
            out.append(from_hist(f"mad_median_{tag}_last_zero_n{n}", "mad", hist, MEDMAD,
                                 lambda F: F.k[0] == F.k[1] and F.t[F.k[0]] == 0 and F.t[F.k[0] + 1] == 2 and (F.keys == 131070).any(),
                                 dict(m2=2 * med, mad4=0), seed=420 + i, tags={"key_131070", "mad_edge"}))
    # half at each end: m2 = -1, both middle keys 65535 (the largest key a rank can have), in MAD bin 511
    for n in mad_lengths(i):
        out.append(from_hist(f"mad_half_half_n{n}", "mad", [(-32768, n // 2), (32767, n // 2)], MEDMAD,
                             lambda F: F.m2 == -1 and (F.keys == 65535).all() and 65535 >> 7 == 511, dict(m2=-1, mad4=131070),
                             seed=430 + i, tags={"max_rank_key"}))
    i += 1
    # the two middle MAD keys on both sides of a 128-key bin edge.  Every key has m2's parity, so the pair is
    # (127, 129) or (255, 257) for an odd m2 -- 127 and 255 are the last keys of their bins -- and (126, 128) or
    # (254, 256) for an even one -- 128 and 256 are the first keys of theirs
    for m2, ka, kb in ((1001, 127, 129), (1000, 126, 128), (-2001, 255, 257), (-2000, 254, 256)):
        for n in mad_lengths(i):
            half = n // 2
            lo_keys = [(ka, 2)] + share((half - 2) // 2, [m2 % 2 + 2, ka - 2, m2 % 2 + 40])
            hi_keys = [(kb, 2)] + share((half - 2) // 2, [kb + 2, kb + 100, 2 * 128 + kb])
            keyh = [(k, 2 * c) if k not in (ka, kb) else (k, c) for k, c in lo_keys + hi_keys]
            assert sum(c for _, c in keyh) == n
            out.append(from_hist(f"mad_bin_edge_{ka}_{kb}_n{n}", "mad", mad_symmetric(m2, keyh), MEDMAD,
                                 lambda F, ka=ka, kb=kb: (int(F.t[F.k[0]]), int(F.t[F.k[1]])) == (ka, kb) and ka >> 7 != kb >> 7
                                 and F.t[F.k[0] - 2] < ka and F.t[F.k[1] + 2] > kb, dict(m2=m2, mad4=ka + kb), seed=440 + i,
                                 tags={"mad_edge"}))
        i += 1
    # more than half the samples at the median: mad4 = 0 and the spread is the floor
    for n in lengths(i):
        m = (3 * n) // 5
        hist = [(431, m)] + share(n - m, [-32768, 200, 430, 432, 700, 32767])
        out.append(from_hist(f"mad_zero_n{n}", "mad", hist, MEDMAD, lambda F: F.t[F.k[1]] == 0 and F.t[-1] > 60000,
                             dict(m2=862, mad4=0), seed=450 + i, tags={"mad_zero"}))
    i += 1
    # the two middle MAD keys in different coarse bins: of one group, and of different groups
    for tag, ka, kb in (("same_group", 100, 300), ("other_group", 100, 1000), ("far_group", 6, 40000)):
        for n in mad_lengths(i):
            half = n // 2
            keyh = [(k, 2 * c) for k, c in share(half // 2, [ka - 6, ka - 2, ka]) + share(half // 2, [kb, kb + 2, kb + 500])]
            out.append(from_hist(f"mad_bins_{tag}_n{n}", "mad", mad_symmetric(500, keyh), MEDMAD,
                                 lambda F, ka=ka, kb=kb, tag=tag: (int(F.t[F.k[0]]), int(F.t[F.k[1]])) == (ka, kb)
                                 and ((ka >> 9 == kb >> 9 and ka >> 7 != kb >> 7) if tag == "same_group" else ka >> 9 != kb >> 9),
                                 dict(m2=500, mad4=ka + kb), seed=460 + i, tags={"mad_bins"}))
        i += 1


# ---- family 5: the one-wave kernel's ends --------------------------------------------------------------------
def _short(out):
    for v in (32767, -32768):
        for n in (1, 64, 449, 512, 513, 1024, 1025):  # the last three: the same reads on the other routes
            out.append(from_hist(f"short_all_{v}_n{n}", "short", [(v, n)], EXTREMES, lambda F, v=v: (F.s == v).all(),
                                 dict(q_lo=v, q_hi=v), tags={"constant_end"}))
    for n in (512, 1024, 2048):
        hist = [(32767 - 64 * i, 1) for i in range(n // 2)] + [(-32768 + 64 * i, 1) for i in range(n // 2)]
        for key, prm in (("extremes", EXTREMES), ("p_hi_1", dict(QUANTILE, p=(0.2, 1.0)))):
            out.append(from_hist(f"short_distinct_{key}_n{n}", "short", hist, prm,
                                 lambda F: np.unique(F.s).size == F.n and F.k[1] == F.n - 1 and F.s[-1] == 32767, dict(q_hi=32767),
                                 seed=500 + n, tags={"distinct_full"}))


# ---- family 6: what a part of a split read holds -------------------------------------------------------------
def part_of(bounds, i):
    return int(np.searchsorted(np.array(bounds), i, side="right")) - 1


def _part(out):
    # every sample of both placed coarse bins lies in one part: the other parts add nothing to the fine histograms
    for n, home in ((3000, 1), (5000, 0), (2049, 1)):
        bounds = parts_of(n)
        b_lo, b_hi, b_mid = 4 * 33 + 2, 4 * 90 + 1, 4 * 60
        kLo, kHi = rank(0.2, n), rank(0.9, n)
        n_lo, n_hi = 40, 50  # the placed bins' samples; the ranks fall among them
        below, above = kLo - n_lo // 2, n - 1 - kHi - n_hi // 2
        mid = n - below - above - n_lo - n_hi
        hist_lo = share(n_lo, [val(b_lo, f) for f in (1, 17, 18, 40, 63)])
        hist_hi = share(n_hi, [val(b_hi, f) for f in (0, 9, 31, 32, 62)])
        rest = share(below, [val(b_lo - 8, 5), val(b_lo - 1, 63)]) + share(mid, [val(b_lo + 1, 0), val(b_mid, 20), val(b_hi - 1, 63)])
        rest += share(above, [val(b_hi + 1, 0), val(b_hi + 40, 7)])
        placed, others = lay(hist_lo + hist_hi, SEED + 600), lay(rest, SEED + 601)
        at = bounds[home] + 13
        x = np.concatenate([others[:at], placed, others[at:]])
        assert at + placed.size < bounds[home + 1]

        def pred(F, bounds=bounds, home=home, b_lo=b_lo, b_hi=b_hi):
            bins = (F.x + 32768) >> 6
            where = {part_of(bounds, i) for i in np.flatnonzero((bins == b_lo) | (bins == b_hi))}
            return where == {home} and len(bounds) - 1 >= 2 and (F.bins(F.k[0])[0], F.bins(F.k[1])[0]) == (b_lo, b_hi)

        out.append(from_hist(f"part_one_home_n{n}", "part", hist_lo + hist_hi + rest, QUANTILE, pred, x=x, tags={"one_home"}))
    # the ranks' only samples among the up to 7 samples before a part's first 16-byte boundary (kLo) and among the
    # up to 7 after its last whole vector (kHi); all values distinct, so a sample scanned twice or not at all moves
    # a rank.  phase: the read's first element, modulo 8 elements; the parts' start phases follow from it
    for start in range(8):  # part 1's start phase
        j = 1
        n = next(m for m in range(2100, 2200) if _edge_slots(m, (start - parts_of(m)[j]) % 8, j) is not None)
        bounds = parts_of(n)
        phase = (start - bounds[j]) % 8
        head_at, tail_at = _edge_slots(n, phase, j)
        c = n // 2
        kLo, kHi = rank(0.2, n), rank(0.9, n)
        x = np.random.default_rng(SEED + 610 + phase).permutation(np.arange(n) - c)
        for k, at in ((kLo, head_at), (kHi, tail_at)):
            i = int(np.flatnonzero(x == k - c)[0])
            x[i], x[at] = x[at], x[i]

        def pred(F, start=start, phase=phase, j=j, head_at=head_at, tail_at=tail_at, bounds=bounds):
            head = (8 - start) % 8
            assert (phase + bounds[j]) % 8 == start
            length = bounds[j + 1] - bounds[j]
            tail = (length - head) % 8
            ok = F.x[head_at] == F.s[F.k[0]] and F.x[tail_at] == F.s[F.k[1]] and np.unique(F.s).size == F.n
            ok = ok and bounds[j + 1] - tail <= tail_at < bounds[j + 1] and tail > 0
            return ok and (bounds[j] <= head_at < bounds[j] + head if head else head_at == bounds[j])

        out.append(from_hist(f"part_head_tail_start{start}", "part", [(i - c, 1) for i in range(n)], QUANTILE, pred,
                             dict(q_lo=kLo - c, q_hi=kHi - c), x=x, phase=phase, tags={"head_tail", f"start{start}"}))
    # sorted reads: each part covers a value range of its own
    n = 4100
    hist = share(n, [val(b, f) for b in (4 * 20 + 3, 4 * 21, 500, 501, 502, 900) for f in (0, 13, 63)])
    up = lay(hist, 0, shuffle=False)
    for tag, x in (("ascending", up), ("descending", up[::-1])):
        for prm_tag, prm in (("quantile", QUANTILE), ("medmad", MEDMAD)):
            out.append(from_hist(f"part_{tag}_{prm_tag}", "part", hist, prm,
                                 lambda F, tag=tag: (np.diff(F.x) >= 0).all() if tag == "ascending" else (np.diff(F.x) <= 0).all(),
                                 x=x, tags={"sorted"}))
    # one multiset twice: the rank's only sample is the last sample of part 0 in one read and the first of part 1
    # in the other, so the parts' own histograms differ by that one sample and their sums do not
    n = 2500
    bounds = parts_of(n)
    c = n // 2
    k = rank(0.2, n)
    base = np.random.default_rng(SEED + 620).permutation(np.arange(n) - c)
    for tag, at in (("last_of_part0", bounds[1] - 1), ("first_of_part1", bounds[1])):
        x = base.copy()
        i = int(np.flatnonzero(x == k - c)[0])
        x[i], x[at] = x[at], x[i]
        out.append(from_hist(f"part_boundary_{tag}", "part", [(i - c, 1) for i in range(n)], QUANTILE,
                             lambda F, at=at: F.x[at] == F.s[F.k[0]] and np.unique(F.s).size == F.n, dict(q_lo=k - c), x=x,
                             tags={"boundary_pair"}))


def _edge_slots(n, phase, j):
    """(an index among part j's head samples -- its first sample where the part starts on a boundary --, an index
    among its tail samples), or None where the part has no tail."""
    bounds = parts_of(n)
    if len(bounds) - 1 <= j:
        return None
    head = (8 - (phase + bounds[j]) % 8) % 8
    length = bounds[j + 1] - bounds[j]
    tail = (length - head) % 8
    if tail == 0:
        return None
    return bounds[j] + (head - 1 if head else 0), bounds[j + 1] - 1 - (tail // 2)


# ---- the catalogue ---------------------------------------------------------------------------------------------
_CAT = None


def catalogue():
    """Every case, built once per process (nothing random but pinned seeds)."""
    global _CAT
    if _CAT is None:
        out = []
        for build in (_edge_coarse, _edge_fine, _pair, _round, _mad, _short, _part):
            build(out)
        names = [c.name for c in out]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
        _CAT = out
    return _CAT


def groups():
    """[(parameters, [cases])]: a call takes one parameter set."""
    by = {}
    for c in catalogue():
        by.setdefault((c.prm["mode"],) + tuple(c.prm["p"]), []).append(c)
    return [(v[0].prm, v) for v in by.values()]


def tagged(tag):
    return [c for c in catalogue() if tag in c.tags]


def pack(cases_or_reads, lead=1):
    """Back to back behind `lead` leading samples (flat, offsets, counts); a case with a phase is moved up to its
    offset modulo 8 by filler samples in front of it."""
    chunks, offsets, at = [np.full(lead, 12345, np.int16)], [], lead
    for c in cases_or_reads:
        x, phase = (c.x, c.phase) if isinstance(c, Case) else (np.asarray(c, np.int16), None)
        if phase is not None and at % 8 != phase:
            pad = (phase - at) % 8
            chunks.append(np.full(pad, -4321, np.int16))
            at += pad
        offsets.append(at)
        chunks.append(x)
        at += x.size
    counts = np.array([(c.x if isinstance(c, Case) else np.asarray(c)).size for c in cases_or_reads], np.int64)
    return np.concatenate(chunks), np.array(offsets, np.int64), counts


# ---- family 7: calls in succession -----------------------------------------------------------------------------
CHAIN_LEVELS, CHAIN_GRID = 64, 1024


def chain_level(r):
    """Consecutive reads, and reads one grid of 1,024 workgroups apart, are one level apart (modulo 64)."""
    return (r + r // CHAIN_GRID) % CHAIN_LEVELS


def chain_bins(r):
    """(placed low bin, heavy bins, placed high bin) of chain read r: the next level's placed bins are this
    level's heavy ones."""
    j = chain_level(r)
    lo, hi = 10 + 5 * j, 1010 - 5 * j
    return lo, (lo + 5, hi - 5), hi


def chain_reads(nreads=1200):
    """Reads of 513 to 600 samples for one call with more reads than the one-workgroup kernel has workgroups: a
    quarter of a read below rank p_lo = 0.2 in one bin, 30% in each of two heavy bins, 15% above p_hi = 0.9."""
    reads = []
    for r in range(nreads):
        n = 513 + (r * 37) % 88
        lo, (a, b), hi = chain_bins(r)
        c_lo, c_a, c_b = n // 4, (3 * n) // 10, (3 * n) // 10
        hist = share(c_lo, [val(lo, (r + f) % 64) for f in (0, 21, 42)]) + share(c_a, [val(a, f) for f in (3, 33)])
        hist += share(c_b, [val(b, f) for f in (7, 57)]) + share(n - c_lo - c_a - c_b, [val(hi, (r + f) % 64) for f in (5, 25, 45)])
        reads.append((lay(hist, SEED + 700 + r), want_of(hist, QUANTILE)))
    return reads


def succession():
    """[(parameters, [(read, want)])] for three calls on one context: med/MAD with 3 split reads, quantiles with 1
    split read of other data, med/MAD with 5."""
    rng = np.random.default_rng(SEED + 800)

    def reads(lengths, lo, hi, prm):
        made = []
        for n in lengths:
            vals = rng.integers(lo, hi, 12)
            hist = share(n, [int(v) for v in vals])
            made.append((lay(hist, SEED + 800 + n), want_of(hist, prm)))
        return made

    return [(MEDMAD, reads([3000, 700, 1025, 2049, 100], -500, 900, MEDMAD)),
            (QUANTILE, reads([64, 4100, 600], 20000, 32768, QUANTILE)),
            (MEDMAD, reads([1500, 2500, 5000, 300, 1026, 4097, 1024], -32768, -30000, MEDMAD))]


# ---- the convert pass --------------------------------------------------------------------------------------------
CONVERT_CHUNKS = [[1, 7, 8], [9, 40, 2100], [2101, 8, 1], [7, 2099, 9, 40], [40], [8, 8, 7, 1, 9]]
CONVERT_GAPS = [3, 1, 6, 2, 5, 4, 7]  # elements in front of read 0, between the reads and behind the last
CONVERT_VIEWS = {  # dtype -> [(out starts this many elements into its allocation, adc likewise or None: in place)]
    "float32": [(1, 0), (2, 3), (3, 5)],
    "float16": [(a, (a + 3) % 8) for a in range(1, 8)] + [(1, None)],
}


def convert_reads():
    """(reads, chunk sizes per read, read_out_offsets, elements the destination needs)."""
    rng = np.random.default_rng(SEED + 900)
    reads = [(rng.normal(500 + 40 * r, 60, sum(cs)).round()).astype(np.int16) for r, cs in enumerate(CONVERT_CHUNKS)]
    starts, at = [], CONVERT_GAPS[0]
    for r, x in enumerate(reads):
        starts.append(at)
        at += x.size + CONVERT_GAPS[r + 1]
    return reads, CONVERT_CHUNKS, np.array(starts, np.int64), at


def byte_phase(dtype, start):
    return (start * (4 if dtype == "float32" else 2)) % 16


# one read of all 65,536 int16 values under three parameter sets: the usual one; a spread so large that every
# output is below binary16's smallest normal number (2^-14); and the floor as spread (p_lo == p_hi gives b - a = 0),
# small enough that (x - centre) / spread passes 65,504 for most x.  With centre_mult 0.5 the centre is the
# integer a and with spread_floor 0.25 the product is the exact integer 4 (x - a): every odd multiple of 2 above
# 2^12 is a binary16 tie
F16_RANGE = {
    "usual": dict(QUANTILE),
    "subnormal": dict(QUANTILE, spread_mult=3.0e4),
    "overflow": dict(QUANTILE, p=(0.5, 0.5), centre_mult=0.5, spread_floor=0.25),
}


def all_values_read():
    return (np.random.default_rng(SEED + 950).permutation(65536).astype(np.int32) - 32768).astype(np.int16)


def f16_ties(v32):
    """Which float32 values lie exactly half-way between two neighbouring binary16 numbers (normal range)."""
    bits = np.ascontiguousarray(v32, np.float32).view(np.uint32)
    a = np.abs(v32)
    return ((bits & np.uint32(0x1FFF)) == np.uint32(0x1000)) & (a >= np.float32(2.0 ** -14)) & (a < np.float32(65520.0))
