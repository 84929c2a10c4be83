"""Heads built for the device trim scan's hazards (tests only, CPU only, numpy).

The device scans 64 windows per step (csrc/pgn_segment.h, trim_scan_wave): lane l takes window g + l, two
ballots give the step's first peak and, from that lane on, its first window whose last sample is not above;
`seen` is carried from step to step.  What decides whether that equals the header's window-by-window rule is
where the peak (P), the stop (Q) and the last whole window (W - 1) fall among the lanes and the steps, so the
heads here place them by construction, not through a generator.

catalogue() gives Case objects that unpack as (name, read int16, trim parameter dict) and carry what they
claim to reach: W windows, P the first window with more than min_elements samples above, Q the first window
at or after P whose last sample is not above, the outcome and the trim, the head statistics m2 and mad4, the
head-size class ("wave": H <= 512, the one-wave selection; "workgroup": H > 1,024, the workgroup selection,
and the selection in parts under set_select_split(1024, 1024, 1024); "none": no statistics taken) and tags.

A designed head is a mask of samples above over a base whose statistics do not move with the mask: the
samples that are not raised hold 90, 100, 110, 100, 90, 100, 110 in turn (3/7 of them at the median), so with
fewer than 3/10 of the head raised twice the median stays 200 and four times the MAD stays 40, and with
mad_mult 1 and threshold_mads 2 the threshold is 120.  Every builder asserts through ref_trim
(tests/test_segment_api.py) that the designed mask is x > thr and that m2 and mad4 are the designed ones; the
claims come from the design, never from ref_trim.

Families: lane (P, Q, W over lanes and steps, at both head sizes), param (parameter edges), thr (threshold
edges), round (a threshold that one rounding and two roundings place on different sides of a sample; the
parameters are searched with a pinned seed), over_n (samples behind max_samples that would move the
statistics), and the heads of test_segment_api.constructed_heads(), taken over unchanged.
"""
from __future__ import annotations

import numpy as np

from test_segment_api import constructed_heads, ref_trim

f32 = np.float32
BASE = (90, 100, 110, 100, 90, 100, 110)
HIGH = 200
UNIT = dict(mad_mult=1.0, threshold_mads=2.0)  # thr = median + 2 MAD: 120 over BASE
WAVE_MAX, SPLIT_MIN = 512, 1024
ROUND_SEED = 20261020

# (W, P, Q, remainder behind the last whole window, samples behind max_samples?)
# remainder: 0, 1 or "max" (window - 1)
PLACEMENTS = [
    (1, 0, 0, 1, False),
    (2, 0, 1, 0, False),          # Q = W - 1 and e == H
    (63, 5, 5, 0, True),
    (64, 5, 9, 1, False),
    (64, 62, 63, 0, False),       # Q = W - 1 and e == H
    (64, 63, 63, 1, False),       # Q = W - 1 with a remainder
    (65, 63, 63, 0, False),
    (65, 63, 64, "max", False),   # Q = W - 1 with a remainder, across the step
    (65, 64, 64, 0, True),        # e == H with samples behind max_samples
    (128, 63, 70, 0, True),
    (129, 64, 65, 1, False),
    (129, 127, 128, 1, False),
    (199, 10, 130, "max", True),
    (199, 130, None, "max", True),
    (63, None, None, 0, True),
    (64, None, None, 1, False),
    (128, None, None, 0, True),
]


class Case:
    def __init__(self, name, family, x, prm, W, P, Q, outcome, trim, m2, mad4, tags=()):
        self.name, self.family = name, family
        self.x = np.ascontiguousarray(x, np.int16)
        self.x.setflags(write=False)
        self.prm = dict(prm)
        self.W, self.P, self.Q, self.outcome, self.trim, self.m2, self.mad4 = W, P, Q, outcome, trim, m2, mad4
        self.tags = set(tags)
        self.H = min(self.x.size, self.prm["max_samples"])
        scanned = self.H >= self.prm["min_trim"] + self.prm["window"]
        self.cls = "none" if not scanned else ("wave" if self.H <= WAVE_MAX else "workgroup")

    def __iter__(self):  # (name, read, trim parameters)
        return iter((self.name, self.x, self.prm))

    def __repr__(self):
        return f"Case({self.name})"


def design_outcome(prm, H, P, Q):
    """(outcome, trim) of a scan with these P and Q, from the header's rule."""
    if P is None:
        return "no_peak", prm["min_trim"]
    if Q is None:
        return "peak_to_end", prm["min_trim"]
    e = prm["min_trim"] + (Q + 1) * prm["window"]
    return ("cut", e) if e < H else ("cut_at_end", prm["min_trim"])


def fill_base(mask, base=BASE):
    """The samples of ~mask take the base values in turn, those of mask HIGH."""
    x = np.full(mask.size, HIGH, np.int64)
    quiet = np.flatnonzero(~mask)
    x[quiet] = np.array(base, np.int64)[np.arange(quiet.size) % len(base)]
    return x.astype(np.int16)


def window_mask(kind, window, mel):
    """One window's samples above.  quiet: none.  decoy: the last and min_elements - 1 more (not a peak).
    peak_go / peak_stop: exactly min_elements + 1, with / without the last.  only_last.  all_but_last.  all."""
    m = np.zeros(window, bool)
    if kind == "decoy":
        assert 1 <= mel <= window
        m[:mel - 1] = True
        m[-1] = True
    elif kind == "peak_go":
        assert mel + 1 <= window
        m[:mel] = True
        m[-1] = True
    elif kind == "peak_stop":
        assert mel + 1 <= window - 1
        m[:mel + 1] = True
    elif kind == "only_last":
        m[-1] = True
    elif kind == "all_but_last":
        m[:-1] = True
    elif kind == "all":
        m[:] = True
    else:
        assert kind == "quiet"
    assert int(m.sum()) == {"decoy": mel, "peak_go": mel + 1, "peak_stop": mel + 1}.get(kind, int(m.sum()))
    return m


def placement_kinds(W, P, Q):
    """The kind of every window of a placement."""
    kinds = []
    decoys = {0, 62, 63, 64, W - 1} | ({P - 1} if P else set())
    for w in range(W):
        if P is None or w < P:
            # mostly windows whose last sample is not above; a few whose last sample is above but that count
            # exactly min_elements
            kinds.append("decoy" if w in decoys else "quiet")
        elif w == P:
            kinds.append("peak_stop" if Q == P else "peak_go")
        elif Q is None or w < Q:
            kinds.append("all" if w % 32 == 7 else "only_last")  # the scan goes on
        elif w == Q:
            kinds.append("all_but_last" if (P + Q) % 2 else "quiet")  # the scan stops
        else:
            kinds.append({1: "only_last", 3: "all_but_last"}.get(w % 16, "quiet"))  # never looked at
    return kinds


def tail_mask(window):
    """What lies behind the last whole window: all above for two windows less one sample, then not above --
    a peak and a stop if windows were formed there."""
    return np.concatenate([np.ones(2 * window - 1, bool), np.zeros(window + 1, bool)])


def build_head(prm, kinds, rem, beyond):
    """(mask of the read, H): min_trim quiet samples, the windows, `rem` samples of the tail inside the head
    and, with beyond, the rest of the tail behind it."""
    window, mel = prm["window"], prm["min_elements"]
    parts = [np.zeros(prm["min_trim"], bool)] + [window_mask(k, window, mel) for k in kinds]
    tail = tail_mask(window)
    assert 0 <= rem < window
    H = prm["min_trim"] + len(kinds) * window + rem
    parts.append(tail if beyond else tail[:rem])
    return np.concatenate(parts), H


def checked(name, family, x, prm, above, W, P, Q, m2, mad4, tags=()):
    """A Case whose design holds on ref_trim's statistics: the mask is x > thr, m2 and mad4 are the designed
    ones.  The outcome and the trim are the design's."""
    x = np.asarray(x, np.int16)
    H = min(x.size, prm["max_samples"])
    with np.errstate(all="ignore"):
        t = ref_trim(x, **prm)
        assert (t["m2"], t["mad4"]) == (m2, mad4), (name, t["m2"], t["mad4"], m2, mad4)
        assert np.array_equal(x[:H].astype(np.float32) > t["thr"], above[:H]), name
    assert W == (H - prm["min_trim"]) // prm["window"], name
    outcome, trim = design_outcome(prm, H, P, Q)
    return Case(name, family, x, prm, W, P, Q, outcome, trim, m2, mad4, tags)


# ---- lane placement ---------------------------------------------------------------------------------------
def size_params(cls, W):
    if cls == "wave":
        if W <= 100:
            return dict(UNIT, window=4, min_elements=2, min_trim=7 if W >= 63 else 40, max_samples=WAVE_MAX)
        if W <= 130:
            return dict(UNIT, window=3, min_elements=1, min_trim=5, max_samples=WAVE_MAX)
        return dict(UNIT, window=2, min_elements=1, min_trim=112, max_samples=WAVE_MAX)  # P == Q cannot be built
    return dict(UNIT, window=40, min_elements=3, min_trim=10 if W >= 63 else 1100, max_samples=8000)


def _lane(out):
    for W, P, Q, rem_spec, beyond in PLACEMENTS:
        for cls in ("wave", "workgroup"):
            prm = size_params(cls, W)
            rem = prm["window"] - 1 if rem_spec == "max" else rem_spec
            kinds = placement_kinds(W, P, Q)
            mask, H = build_head(prm, kinds, rem, beyond)
            if beyond:
                prm["max_samples"] = H
            assert H <= prm["max_samples"] and (H <= WAVE_MAX if cls == "wave" else H > SPLIT_MIN)
            tags = {"lane"}
            if P is not None and P % 64:
                tags.add("mask")  # windows of the peak's step in front of it are not above
            if P is not None and Q is not None and P // 64 != Q // 64:
                tags.add("step_boundary")
            if P is not None and Q is None and W > 64 * (P // 64 + 1):
                tags.add("step_boundary")
            if Q is not None and prm["min_trim"] + (Q + 1) * prm["window"] == H:
                tags.add("e_eq_H")
            if Q is not None and Q == W - 1 and rem:
                tags.add("last_window_remainder")
            if beyond:
                tags.add("behind_max_samples")
            if "decoy" in kinds[:P]:
                tags.add("decoy")
            name = f"lane_W{W}_P{P}_Q{Q}_{cls}"
            c = checked(name, "lane", fill_base(mask), prm, mask, W, P, Q, 200, 40, tags)
            assert c.cls == cls
            out.append(c)


# ---- parameter edges ----------------------------------------------------------------------------------------
def _from_kinds(out, name, family, prm, kinds, P, Q, rem=0, beyond=False, tags=()):
    mask, H = build_head(prm, kinds, rem, beyond)
    assert H == min(mask.size, prm["max_samples"])
    out.append(checked(name, family, fill_base(mask), prm, mask, (H - prm["min_trim"]) // prm["window"], P, Q, 200, 40, tags))


def _param(out):
    q = "quiet"
    # window 1, min_elements 0: the count is the last sample
    k = [q] * 20 + ["all"] * 5 + [q] * 60
    _from_kinds(out, "param_window1_mel0", "param", dict(UNIT, window=1, min_elements=0, min_trim=3, max_samples=400),
                k, 20, 25)
    # window 1, min_elements 1: never a peak
    _from_kinds(out, "param_window1_mel1", "param", dict(UNIT, window=1, min_elements=1, min_trim=3, max_samples=400),
                k, None, None)
    # min_elements >= window: windows that are all above are no peak
    for mel in (4, 9):
        k4 = [q] * 3 + ["all", "all_but_last"] + [q] * 30
        _from_kinds(out, f"param_mel{mel}_window4", "param",
                    dict(UNIT, window=4, min_elements=mel, min_trim=7, max_samples=400), k4, None, None)
    # min_trim 0
    k0 = [q, "decoy", "peak_go", "all_but_last"] + [q] * 40
    _from_kinds(out, "param_min_trim0", "param", dict(UNIT, window=4, min_elements=2, min_trim=0, max_samples=400),
                k0, 2, 3, rem=1)
    # H == min_trim + window: one window, e == H
    one = dict(UNIT, window=40, min_elements=3, min_trim=10, max_samples=8000)
    _from_kinds(out, "param_one_window_n", "param", one, ["peak_stop"], 0, 0, tags={"e_eq_H"})
    _from_kinds(out, "param_one_window_max_samples", "param", dict(one, max_samples=50), ["peak_stop"], 0, 0,
                beyond=True, tags={"e_eq_H", "behind_max_samples"})
    # H == min_trim + window - 1: no window
    short = fill_base(np.concatenate([np.zeros(10, bool), np.ones(39, bool)]))
    out.append(Case("param_no_window", "param", short, one, 0, None, None, "no_window", 10, 0, 0))
    out.append(Case("param_no_window_max_samples", "param", np.concatenate([short, short]), dict(one, max_samples=49), 0,
                    None, None, "no_window", 10, 0, 0, {"behind_max_samples"}))
    # n < min_trim: the trim is n
    out.append(Case("param_n_below_min_trim", "param", short[:6], one, 0, None, None, "no_window", 6, 0, 0))
    out.append(Case("param_empty", "param", short[:0], one, 0, None, None, "no_window", 0, 0, 0))
    # max_samples 1: one window of one sample, which is its own median
    x1 = np.array([150, 300, 90, 100, 110, 100, 90, 100], np.int16)
    p1 = dict(UNIT, window=1, min_elements=0, min_trim=0, max_samples=1)
    out.append(checked("param_max_samples1", "param", x1, p1, np.zeros(1, bool), 1, None, None, 300, 0,
                       {"behind_max_samples"}))
    out.append(Case("param_max_samples1_no_window", "param", x1, dict(one, max_samples=1), 0, None, None, "no_window", 8,
                    0, 0, {"behind_max_samples"}))
    # max_samples > n
    ku = [q, "decoy", q, "peak_go", "only_last", "all_but_last", q]
    _from_kinds(out, "param_max_samples_above_n", "param", one, ku, 3, 5, rem=17)
    # window 3,000 with two windows: one lane runs the long loop
    long_w = dict(UNIT, window=3000, min_elements=3, min_trim=10, max_samples=8000)
    _from_kinds(out, "param_window3000", "param", long_w, ["peak_go", "quiet"], 0, 1, rem=490, tags={"long_window"})
    _from_kinds(out, "param_window3000_end", "param", long_w, ["decoy", "peak_stop"], 1, 1, tags={"long_window", "e_eq_H"})


# ---- threshold edges ----------------------------------------------------------------------------------------
def _thr(out):
    q = "quiet"
    geo = dict(window=4, min_elements=2, min_trim=7, max_samples=400)
    kinds = [q, "decoy", q, "peak_go", "only_last", "all_but_last"] + [q] * 30
    mask, H = build_head(dict(geo), kinds, 3, False)
    x = fill_base(mask)
    W = (H - 7) // 4
    every = np.ones(H, bool)
    none = np.zeros(H, bool)
    # negative threshold_mads: everything is above (thr = 100 - 20 * 10)
    out.append(checked("thr_negative_mads", "thr", x, dict(geo, mad_mult=1.0, threshold_mads=-20.0), every, W, 0, None,
                       200, 40))
    # threshold_mads so large that nothing is above
    out.append(checked("thr_huge_mads", "thr", x, dict(geo, mad_mult=1.0, threshold_mads=1e6), none, W, None, None, 200, 40))
    # the spread overflows: thr = +inf, -inf, and 0 * inf = NaN (nothing is above a NaN)
    for tag, tm, above, P in (("plus_inf", 2.0, none, None), ("minus_inf", -2.0, every, 0), ("nan", 0.0, none, None)):
        c = checked(f"thr_{tag}", "thr", x, dict(geo, mad_mult=3e38, threshold_mads=tm), above, W, P, None, 200, 40,
                    {"nonfinite_thr"})
        with np.errstate(all="ignore"):
            thr = ref_trim(x, **c.prm)["thr"]
        assert {"plus_inf": thr == np.inf, "minus_inf": thr == -np.inf, "nan": np.isnan(thr)}[tag]
        out.append(c)
    # mad4 == 0: more than half the head at the median; thr == centre and equal is not above
    flat = np.where(mask, HIGH, 100).astype(np.int16)
    out.append(checked("thr_mad0", "thr", flat, dict(geo, **UNIT), mask, W, 3, 5, 200, 0))
    one_up = flat.copy()
    one_up[7:11] = 101  # window 0: four samples just above the centre -- a peak, and its last sample is above
    m1 = mask.copy()
    m1[7:11] = True
    out.append(checked("thr_mad0_one_above_centre", "thr", one_up, dict(geo, **UNIT), m1, W, 0, 2, 200, 0))
    # a half-integer centre: H even, half the head at 100 and below, half at 101 and above (m2 = 201, mad4 = 2,
    # thr = 100.5 + 2 * 0.5 = 101.5): 101 is not above, 102 is
    assert H % 2 == 0
    half = np.full(H, 100, np.int64)
    quiet = np.flatnonzero(~mask)
    half[quiet[quiet.size - (H // 2 - int(mask.sum())):]] = 101
    half[mask] = 102
    assert int((half == 100).sum()) == H // 2
    out.append(checked("thr_half_integer_centre", "thr", half, dict(geo, **UNIT), mask, W, 3, 5, 201, 2))
    # a sample equal to the threshold: windows that would be peaks if 120 counted as above
    eq = x.copy()
    eq[mask] = 120
    out.append(checked("thr_equal_is_not_above", "thr", eq, dict(geo, **UNIT), none, W, None, None, 200, 40, {"tie"}))
    mix = x.copy()
    mix[7 + 3 * 4] = 120  # window 3 keeps two samples above and one equal: min_elements, so window 5 is the peak
    mm = mask.copy()
    mm[7 + 3 * 4] = False
    out.append(checked("thr_equal_in_the_peak", "thr", mix, dict(geo, **UNIT), mm, W, 5, 5, 200, 40, {"tie"}))
    # heads at the ends of int16
    lo = np.where(mask, 32767, -32768).astype(np.int16)
    out.append(checked("thr_int16_min_head", "thr", lo, dict(geo, **UNIT), mask, W, 3, 5, -65536, 0))
    hi = np.where(mask, -32768, 32767).astype(np.int16)
    out.append(checked("thr_int16_max_head", "thr", hi, dict(geo, **UNIT), none, W, None, None, 65534, 0))


# ---- one rounding or two ----------------------------------------------------------------------------------
def thresholds(m2, mad4, mad_mult, threshold_mads):
    """(thr as the header defines it, thr with the product and the sum rounded once): float32."""
    centre = f32(0.5) * f32(m2)
    spread = f32(mad_mult) * (f32(0.25) * f32(mad4))
    two = centre + f32(threshold_mads) * spread
    once = f32(np.float64(centre) + np.float64(f32(threshold_mads)) * np.float64(spread))
    return two, once


def search_rounding():
    """Parameters, found with a pinned seed, for which the two thresholds differ and one of them is an integer
    v.  Double rounding differs from single rounding only through a tie, and ties go to even, so the integer is
    always the header's (two-rounding) value.  "two_above": once < two == v, so the sample v lies between
    them -- not above by the header's rule, above after one rounding.  "two_below": v == two < once, where no
    int16 lies between them and only the threshold's bits tell the two apart.  The head's base is c - d, c,
    c + d."""
    rng = np.random.default_rng(ROUND_SEED)
    N = 1 << 21
    c = rng.integers(8000, 12000, N)
    d = rng.integers(20, 400, N)
    mm = rng.uniform(1.0, 2.0, N).astype(np.float32)
    tm = rng.uniform(1.5, 4.0, N).astype(np.float32)
    centre = f32(0.5) * (2 * c).astype(np.float32)
    spread = mm * (f32(0.25) * (4 * d).astype(np.float32))
    two = centre + tm * spread
    once = (centre.astype(np.float64) + tm.astype(np.float64) * spread.astype(np.float64)).astype(np.float32)
    hit = (two != once) & (two == np.floor(two)) & (two < 32000) & (two > (c + d))
    found = {}
    for i in np.flatnonzero(hit):
        key = "two_below" if two[i] < once[i] else "two_above"
        if key not in found:
            found[key] = (int(c[i]), int(d[i]), float(mm[i]), float(tm[i]), int(two[i]))
    assert set(found) == {"two_below", "two_above"}, found
    return found


def _round(out):
    q = "quiet"
    geo = dict(window=4, min_elements=2, min_trim=7, max_samples=400)
    kinds = [q, "decoy", q, "peak_go", "only_last", "all_but_last"] + [q] * 30
    mask, H = build_head(dict(geo), kinds, 2, False)
    W = (H - 7) // 4
    for key, (c, d, mm, tm, v) in search_rounding().items():
        prm = dict(geo, mad_mult=mm, threshold_mads=tm)
        two, once = thresholds(2 * c, 4 * d, mm, tm)
        assert two != once and two == v and (once < v if key == "two_above" else once > v)
        x = fill_base(mask, base=tuple(c + (b - 100) // 10 * d for b in BASE))
        if key == "two_above":  # the raised samples are v itself: nothing is above
            x[mask] = v
            out.append(checked(f"round_{key}", "round", x, prm, np.zeros(H, bool), W, None, None, 2 * c, 4 * d,
                               {"rounding", "sample_between"}))
        else:  # v + 1 is above either way
            x[mask] = v + 1
            out.append(checked(f"round_{key}", "round", x, prm, mask, W, 3, 5, 2 * c, 4 * d, {"rounding"}))


# ---- samples behind max_samples that would move the statistics ----------------------------------------------
def _over_n(out):
    q = "quiet"
    prm = dict(UNIT, window=4, min_elements=2, min_trim=7, max_samples=151)
    kinds = [q, "decoy", q, "peak_go", "only_last", "all_but_last"] + [q] * 30
    mask, H = build_head(prm, kinds, 0, False)
    assert H == 151
    x = np.concatenate([fill_base(mask), np.full(3 * H, 1000, np.int16)])
    out.append(checked("over_n_high_tail", "over_n", x, prm, mask, 36, 3, 5, 200, 40, {"behind_max_samples"}))
    big = dict(UNIT, window=40, min_elements=3, min_trim=10, max_samples=1500)
    mask, H = build_head(big, kinds + [q], 10, False)
    assert H == 1500
    x = np.concatenate([fill_base(mask), np.full(3 * H, 1000, np.int16)])
    out.append(checked("over_n_high_tail_workgroup", "over_n", x, big, mask, 37, 3, 5, 200, 40, {"behind_max_samples"}))


# ---- the heads of tests/test_segment_api.py -------------------------------------------------------------------
CONSTRUCTED = {  # name -> W, P, Q, outcome, trim, m2, mad4
    "constant": (7, None, None, "no_peak", 10, -154, 0),
    "all_max": (199, None, None, "no_peak", 10, 65534, 0),
    "threshold_tie": (4, None, None, "no_peak", 10, 200, 40),
    "plateau": (9, 1, 2, "cut", 130, 1000, 0),
}


def _constructed(out):
    for name, x, prm in constructed_heads():
        out.append(Case(f"constructed_{name}", "constructed", x, prm, *CONSTRUCTED[name], tags={"tie"} if "tie" in name else ()))


_CAT = None


def catalogue():
    """Every case, built once per process (nothing random but the pinned search)."""
    global _CAT
    if _CAT is None:
        out = []
        for build in (_lane, _param, _thr, _round, _over_n, _constructed):
            build(out)
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        _CAT = out
    return _CAT


def groups():
    """[(trim parameters, [cases])]: the C ABI takes one pgn_trim_params per call."""
    by = {}
    for c in catalogue():
        by.setdefault(tuple(sorted(c.prm.items())), []).append(c)
    return [(dict(k), v) for k, v in by.items()]


def tagged(tag):
    return [c for c in catalogue() if tag in c.tags]

