"""The heads of tests/_trim_cases.py check themselves (CPU): every case's claim -- W, P, Q, the outcome, the
trim, the head statistics and the head-size class -- holds on ref_trim; the host build of the scan
(libpgn_model.so) and the NumPy mirror (trim_signal) agree with it on every case; and a restatement of the
rule in the device's shape (64 windows per step, a peak ballot, a stop ballot and a mask), given one named
fault at a time, shows that the set tells each fault from the true rule.  That last check is what says the set
would notice a subtly wrong kernel, and it needs no GPU.
"""
import collections

import numpy as np
import pytest

import _trim_cases as T
from test_norm_api import ref_medmad
from test_segment_api import assert_trim_equal, model_trim, needs_model, ref_trim

CAT = T.catalogue


def ref(c):
    with np.errstate(all="ignore"):  # the spread overflows on purpose in the non-finite cases
        return ref_trim(c.x, **c.prm)


def scan_facts(x, thr, H, window, min_elements, min_trim, **_):
    """(W, P, Q) of a head from its samples and ref_trim's threshold, by the claims' definitions."""
    with np.errstate(invalid="ignore"):
        above = x[:H].astype(np.float32) > thr
    W = (H - min_trim) // window
    win = above[min_trim:min_trim + W * window].reshape(W, window)
    peaks = np.flatnonzero(win.sum(axis=1) > min_elements)
    P = int(peaks[0]) if peaks.size else None
    Q = None
    if P is not None:
        stops = np.flatnonzero(~win[P:, -1])
        Q = P + int(stops[0]) if stops.size else None
    return W, P, Q


def test_every_claim_holds_on_the_reference():
    for c in CAT():
        t = ref(c)
        assert (t["trim"], t["outcome"]) == (c.trim, c.outcome), (c.name, t, c.trim, c.outcome)
        assert (t["m2"], t["mad4"]) == (c.m2, c.mad4), (c.name, t)
        if c.cls == "none":
            assert c.outcome == "no_window" and c.H < c.prm["min_trim"] + c.prm["window"], c.name
            assert c.trim == min(c.prm["min_trim"], c.x.size) and (c.W, c.P, c.Q) == (0, None, None), c.name
            continue
        assert scan_facts(c.x, t["thr"], c.H, **c.prm) == (c.W, c.P, c.Q), c.name
        assert (c.H <= T.WAVE_MAX) if c.cls == "wave" else (c.H > T.SPLIT_MIN), (c.name, c.H)
        assert c.H == min(c.x.size, c.prm["max_samples"])
        # the claims are consistent with the header's rule
        assert T.design_outcome(c.prm, c.H, c.P, c.Q) == (c.outcome, c.trim), c.name


def test_the_placements_the_issue_lists():
    lane = [c for c in CAT() if c.family == "lane"]
    for cls in ("wave", "workgroup"):
        have = {(c.W, c.P, c.Q) for c in lane if c.cls == cls}
        assert {w for w, _, _ in have} == {1, 2, 63, 64, 65, 128, 129, 199}, cls
        want = {(0, 0), (0, 1), (5, 5), (5, 9), (62, 63), (63, 63), (63, 64), (63, 70), (64, 64), (64, 65), (10, 130),
                (127, 128), (130, None), (None, None)}
        assert {(p, q) for _, p, q in have} == want, cls
        for tag in ("mask", "step_boundary", "e_eq_H", "last_window_remainder", "behind_max_samples", "decoy"):
            assert any(tag in c.tags and c.cls == cls for c in lane), (cls, tag)
        # Q = W - 1 once with e == H (the rule returns min_trim) and once with a remainder behind it
        assert any(c.Q == c.W - 1 and c.outcome == "cut_at_end" for c in lane if c.cls == cls)
        assert any(c.Q == c.W - 1 and c.outcome == "cut" and c.H > c.trim for c in lane if c.cls == cls)
    # what the tags say, on the claims
    for c in T.tagged("mask"):
        assert c.P % 64 > 0
    for c in T.tagged("step_boundary"):
        assert c.P // 64 < (c.Q if c.Q is not None else c.W - 1) // 64
    for c in T.tagged("e_eq_H"):
        assert c.prm["min_trim"] + (c.Q + 1) * c.prm["window"] == c.H and c.outcome == "cut_at_end"
    for c in T.tagged("behind_max_samples"):
        assert c.x.size > c.H
    outcomes = collections.Counter(c.outcome for c in CAT())
    assert set(outcomes) == {"no_window", "cut", "no_peak", "peak_to_end", "cut_at_end"}, outcomes


def test_the_edges_the_issue_lists():
    by = {c.name: c for c in CAT()}
    prm = lambda n: by[n].prm
    assert (prm("param_window1_mel0")["window"], prm("param_window1_mel0")["min_elements"]) == (1, 0)
    assert by["param_window1_mel0"].outcome == "cut" and by["param_window1_mel1"].outcome == "no_peak"
    assert all(by[n].prm["min_elements"] >= by[n].prm["window"] for n in ("param_mel4_window4", "param_mel9_window4"))
    assert prm("param_min_trim0")["min_trim"] == 0 and by["param_min_trim0"].trim == 16
    for n in ("param_one_window_n", "param_one_window_max_samples"):
        assert by[n].H == prm(n)["min_trim"] + prm(n)["window"] and by[n].W == 1 and by[n].outcome == "cut_at_end"
    assert by["param_no_window"].H == prm("param_no_window")["min_trim"] + prm("param_no_window")["window"] - 1
    assert by["param_n_below_min_trim"].trim == by["param_n_below_min_trim"].x.size == 6
    assert by["param_max_samples1"].H == 1 and by["param_max_samples1"].W == 1
    assert prm("param_max_samples_above_n")["max_samples"] > by["param_max_samples_above_n"].x.size
    assert prm("param_window3000")["window"] == 3000 and by["param_window3000"].W == 2
    thr = {n: ref(by[n])["thr"] for n in by}
    assert thr["thr_plus_inf"] == np.inf and thr["thr_minus_inf"] == -np.inf and np.isnan(thr["thr_nan"])
    assert by["thr_minus_inf"].outcome == by["thr_negative_mads"].outcome == "peak_to_end"
    assert by["thr_mad0"].mad4 == 0 and float(thr["thr_mad0"]) == 100.0 and (by["thr_mad0"].x == 100).sum() > 77
    assert by["thr_half_integer_centre"].m2 % 2 == 1 and float(thr["thr_half_integer_centre"]) == 101.5
    assert (by["thr_equal_is_not_above"].x == 120).sum() > 5 and float(thr["thr_equal_is_not_above"]) == 120.0
    assert by["thr_int16_min_head"].x.min() == -32768 and by["thr_int16_max_head"].x.max() == 32767
    assert float(thr["thr_int16_min_head"]) == -32768.0 and float(thr["thr_int16_max_head"]) == 32767.0
    for n in ("round_two_above", "round_two_below"):
        c = by[n]
        two, once = T.thresholds(c.m2, c.mad4, c.prm["mad_mult"], c.prm["threshold_mads"])
        assert two.view(np.uint32) == thr[n].view(np.uint32) and two != once, n
    c = by["round_two_above"]
    two, once = T.thresholds(c.m2, c.mad4, c.prm["mad_mult"], c.prm["threshold_mads"])
    between = c.x[(c.x.astype(np.float32) > once) & ~(c.x.astype(np.float32) > two)]
    assert between.size >= 3, "no sample lies between the two thresholds"


@needs_model
def test_host_model_on_every_case():
    for c in CAT():
        assert_trim_equal(model_trim(c.x, **c.prm), ref(c), c.name)


def test_numpy_mirror_on_every_case():
    from rawnanoporesignalcompression_amd import trim_signal

    for c in CAT():
        with np.errstate(all="ignore"):
            assert trim_signal(c.x, **c.prm) == c.trim, c.name


# ---- the rule in the device's shape, with one optional fault ------------------------------------------------
FAULTS = {
    "equal_is_above": "a sample equal to the threshold counts as above",
    "peak_at_min_elements": "a window with exactly min_elements samples above is a peak",
    "stop_before_peak": "the first not-above window of the peak's 64-window step is taken even in front of P",
    "seen_dropped": "seen is forgotten at a 64-window boundary",
    "peak_cannot_stop": "the peak's own window cannot stop the scan",
    "windows_past_W": "windows are formed, and the end of the head is taken, from n instead of min(n, max_samples)",
    "e_at_end": "trim_at returns e where e == H",
    "stats_over_n": "the statistics are taken over n samples instead of min(n, max_samples)",
    "round_once": "the threshold's product and sum are rounded once (an FMA)",
}


def wave_rule(x, fault=None, *, max_samples, window, min_elements, min_trim, mad_mult, threshold_mads):
    """The trim by the device's plan: 64 windows per step, the step's first peak, the step's first stop at or
    behind it, seen carried on.  fault: one of FAULTS."""
    x = np.asarray(x, np.int16)
    n = x.size
    if max_samples == 0:
        return 0
    H = min(n, max_samples)
    if H < min_trim + window:
        return min(min_trim, n)
    m2, mad4 = ref_medmad(x if fault == "stats_over_n" else x[:H])
    with np.errstate(all="ignore"):
        two, once = T.thresholds(m2, mad4, mad_mult, threshold_mads)
        thr = once if fault == "round_once" else two
        xf = x.astype(np.float32)
        above = xf >= thr if fault == "equal_is_above" else xf > thr
    end = n if fault == "windows_past_W" else H
    W = (end - min_trim) // window
    win = above[min_trim:min_trim + W * window].reshape(W, window)
    cnt, last = win.sum(axis=1), win[:, -1]
    peak = cnt >= min_elements if fault == "peak_at_min_elements" else cnt > min_elements

    def trim_at(w):
        e = min_trim + (w + 1) * window
        return e if (e <= end if fault == "e_at_end" else e < end) else min_trim

    seen = False
    for g in range(0, W, 64):
        lanes = np.arange(g, min(g + 64, W))
        if fault == "seen_dropped":
            seen = False
        stop = lanes[~last[lanes]]
        if not seen:
            peaks = lanes[peak[lanes]]
            if not peaks.size:
                continue
            seen = True
            if fault == "peak_cannot_stop":
                stop = stop[stop > peaks[0]]
            elif fault != "stop_before_peak":
                stop = stop[stop >= peaks[0]]
        if stop.size:
            return trim_at(int(stop[0]))
    return min_trim


def test_restatement_agrees_with_the_reference():
    for c in CAT():
        assert wave_rule(c.x, **c.prm) == c.trim, c.name


@pytest.mark.parametrize("fault", list(FAULTS))
def test_every_fault_is_caught(fault):
    """A scan with this fault gives another trim than the reference on at least one case."""
    caught = [c.name for c in CAT() if wave_rule(c.x, fault, **c.prm) != c.trim]
    print(fault, len(caught), caught[:8])
    assert caught, FAULTS[fault]


def test_faults_are_caught_at_both_head_sizes():
    """The scan faults (not those of the statistics or the threshold, which have cases of their own) are caught
    by a lane case of each head-size class, so the GPU run meets them behind every selection kernel."""
    for fault in ("peak_at_min_elements", "stop_before_peak", "seen_dropped", "peak_cannot_stop", "windows_past_W",
                  "e_at_end"):
        for cls in ("wave", "workgroup"):
            assert any(wave_rule(c.x, fault, **c.prm) != c.trim for c in CAT() if c.family == "lane" and c.cls == cls), (fault, cls)
