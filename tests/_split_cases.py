"""Signals built for the split's windows and seams, for every encoder route (tests only, CPU only).

The device split is not the reference's loop: a step is 1,024 samples and a lane takes 16 of them, the
deltas and classes come from packed 16-bit halves, the places from one packed wave scan (fields of 11,
11 and 10 bits), the bytes go through LDS windows that carry a tail from step to step and leave as
16-byte blocks, and small batches split a chunk over 32 single-wave ranges that start in the middle of
a block and share S bytes.  A wrong bound in any of it still writes a well-formed blob, so only byte
identity with the oracle sees it, and only on a signal that reaches the bound.

A chunk here is built from its zig-zag deltas, x[i] = x[i-1] + unzigzag(z[i]) in 16-bit wrap-around
with x[-1] = 0, so a case chooses the class of every sample.  Values are position-coded (coded()): the
k-th entry of a stream carries k, so a dropped, repeated, stale or misplaced byte shows.

catalogue() -> the cases (families values, seams, counts, carries, ragged, ranges, capacity), each with
the codecs it is meant for and claims: statements about split_shape(), the plain numpy model of the
fills, blocks and ranges over the oracle's classes.  split_as_device() restates the split in the
device's shape, per step and lane, and takes one named fault at a time (FAULTS);
tests/test_split_cases.py holds it to the oracle without a fault and shows that every fault changes the
streams of some case.
"""
from __future__ import annotations

import numpy as np

import _oracle as O

CODECS = ["C5", "C4", "C1", "C2", "C3", "VBZ0", "VBZ"]
FIVE = ("C5", "C4")
ONE_BIT = ("C1", "C2", "C3", "VBZ")
FAMILIES = ["values", "seams", "counts", "carries", "ragged", "ranges", "capacity"]
STEP = 1024
RANGES = 32
PASS_SAMPLES = 262144
THRESHOLDS = [0, 1, 2, 15, 16, 17, 18, 255, 256, 257, 271, 272, 273, 274, 65534, 65535]

# fault -> the codecs whose split has the part that goes wrong (the range split is C5's alone)
FAULTS = {
    "field3_wrap": FIVE,
    "lane0_prev": tuple(CODECS),
    "range_prev": ("C5",),
    "half_borrow": FIVE,
    "threshold_ge": FIVE,
    "tail_keys": tuple(CODECS),
    "odd_nibble_high": ("C5", "C4", "VBZ0"),
    "carry_dropped": ("C5", "C4", "C1", "VBZ0", "VBZ"),
    "full_window_63": FIVE,
    "lead_written": ("C5",),
    "odd_lead_byte": ("C5",),
    "empty_range_owner": ("C5",),
    "last_half_owner": ("C5",),
    "late_first_entry": ("C5",),
}
RANGE_FAULTS = ("range_prev", "lead_written", "odd_lead_byte", "empty_range_owner", "last_half_owner",
                "late_first_entry")


# ---- signals from classes ---------------------------------------------------------------------------
def unzigzag(z):
    z = np.asarray(z, np.int64)
    return (z >> 1) ^ -(z & 1)


def signal(z):
    """x[i] = x[i-1] + unzigzag(z[i]) mod 2^16, x[-1] = 0"""
    z = np.asarray(z, np.int64)
    assert z.size == 0 or (0 <= z.min() and z.max() <= 65535)
    return (np.cumsum(unzigzag(z)) & 0xFFFF).astype(np.uint16).view(np.int16)


def zigzag_of(x):
    """the zig-zag deltas of a signal (what every split computes first)"""
    u = np.asarray(x, np.int16).view(np.uint16).astype(np.int64)
    d = (u - np.concatenate([[0], u[:-1]])) & 0xFFFF
    return ((d << 1) ^ -(d >> 15)) & 0xFFFF


def coded(cls, kind="C5"):
    """zig-zag values for the classes `cls` (0..3), the k-th entry of a stream carrying k"""
    cls = np.asarray(cls, np.int64)
    lo1, lo2, lo3 = (1, 17, 273) if kind == "C5" else (1, 16, 256)
    z = np.zeros(cls.size, np.int64)
    for c in (1, 2, 3):
        idx = np.flatnonzero(cls == c)
        k = np.arange(idx.size)
        if c == 1:
            z[idx] = lo1 + k % 13
        elif c == 2:
            z[idx] = lo2 + k % (251 if kind == "C5" else 239)
        else:
            z[idx] = lo3 + k % 253 + 256 * ((k // 253) % 241)
    return z


def range_plan(n):
    """[(t0, t1)] of the 32 ranges of a chunk: s0 = steps * r / 32"""
    steps = (n + STEP - 1) // STEP
    out = []
    for r in range(RANGES):
        s0, s1 = steps * r // RANGES, steps * (r + 1) // RANGES
        out.append((s0 * STEP, min(s1 * STEP, n)))
    return out


class Case:
    def __init__(self, name, x, codecs=None, claims=None):
        self.name, self.family = name, name.split("/")[0]
        assert self.family in FAMILIES
        self.x = np.ascontiguousarray(x, np.int16)
        self.n = self.x.size
        self.codecs = tuple(codecs or CODECS)
        self.claims = dict(claims or {})  # text -> (codec, predicate over split_shape(x, codec))

    def __repr__(self):
        return f"Case({self.name}, n={self.n})"


# ---- the oracle's streams and classes -----------------------------------------------------------------
def oracle_streams(x, codec):
    if codec == "C5":
        return O.c5_streams(x)
    if codec == "VBZ":
        return [O.oracle_vbz_svb_encode(x)]
    return O.variant_streams(codec, x)


def ref_streams(x, codec):
    if codec == "VBZ":
        return [O.ref_vbz_svb_encode(x)]
    return O.ref_variant_streams(codec, x)


def oracle_classes(x, codec):
    """the class of every sample as the oracle's keys state it (2-bit codes, or the 1-bit big flag)"""
    n = np.asarray(x).size
    keys = np.frombuffer(oracle_streams(x, codec)[0], np.uint8)
    if codec in FIVE or codec == "VBZ0":
        k = keys[: (n + 3) // 4].astype(np.int64)
        return ((k[:, None] >> (2 * np.arange(4))) & 3).reshape(-1)[:n]
    k = keys[: (n + 7) // 8]
    return np.unpackbits(k, bitorder="little")[:n].astype(np.int64)


# ---- shape model ----------------------------------------------------------------------------------------
def _window(before, add, unit):
    fill = before + add
    return {"before": before, "add": add, "fill": fill, "blocks": fill // unit, "after": fill % unit}


def split_shape(x, codec):
    """Plain numpy over the oracle's classes: per step the class counts, every window's fill before and after
    and the blocks that leave; for C5 per range t0, t1, the three start offsets, whether it holds nibbles, and
    the owners (low nibble's range, high nibble's range) of every S byte two ranges share."""
    x = np.asarray(x, np.int16)
    n = x.size
    cls = oracle_classes(x, codec)
    steps = []
    fS = fM = fL = fD = fN = 0
    for t in range(0, n, STEP):
        c = cls[t:t + STEP]
        s = {"t": t, "full": t + STEP <= n, "samples": c.size}
        if codec in FIVE:
            n1, n2, n3 = (int((c == k).sum()) for k in (1, 2, 3))
            s.update(n1=n1, n2=n2, n3=n3, S=_window(fS, n1, 32), M=_window(fM, n2, 16), L=_window(fL, n3, 16))
            s["field3_wraps"] = n3 >= 1024
            fS, fM, fL = s["S"]["after"], s["M"]["after"], s["L"]["after"]
        elif codec == "VBZ0":
            nib = int(((c == 1) + 2 * (c == 2) + 4 * (c == 3)).sum())
            s.update(nibbles=nib, N=_window(fN, nib, 32))
            fN = s["N"]["after"]
        else:
            big = int(c.sum())
            s.update(big=big, small=c.size - big, D=_window(fD, c.size + big, 16))
            fD = s["D"]["after"]
        steps.append(s)
    out = {"n": n, "steps": steps, "classes": cls}
    if codec in FIVE:
        out["totals"] = tuple(int((cls == k).sum()) for k in (1, 2, 3))
    if codec == "C5":
        ranges, pS, pM, pL = [], 0, 0, 0
        for r, (t0, t1) in enumerate(range_plan(n)):
            c = cls[t0:t1] if t0 < t1 else cls[:0]
            cS, cM, cL = (int((c == k).sum()) for k in (1, 2, 3))
            first_step = None
            for j, t in enumerate(range(t0, t1, STEP)):
                if (cls[t:min(t + STEP, t1)] == 1).any():
                    first_step = j
                    break
            ranges.append({"r": r, "t0": t0, "t1": t1, "empty": t0 >= t1, "steps": max(0, -(-(t1 - t0) // STEP)),
                           "pS": pS, "pM": pM, "pL": pL, "cS": cS, "cM": cM, "cL": cL, "nibbles": cS > 0,
                           "first_nibble_step": first_step})
            pS, pM, pL = pS + cS, pM + cM, pL + cL
        shared, at, last = {}, 0, None
        for g in ranges:
            if not g["nibbles"]:
                continue
            if at & 1 and last is not None:
                shared[at >> 1] = (last, g["r"])
            at += g["cS"]
            last = g["r"]
        out.update(ranges=ranges, shared=shared, trailing_owner=last if at & 1 else None)
    return out


# ---- the split restated in the device's shape ---------------------------------------------------------------
def _zz(d):
    d = d & 0xFFFF
    return ((d << 1) ^ -(d >> 15)) & 0xFFFF


class _Walk:
    """the state one wave carries from step to step"""

    def __init__(self, x, n, fault):
        self.x, self.n, self.fault = x, n, fault
        self.prevX, self.done = 0, 0

    def deltas(self, t, packed):
        """the 1,024 zig-zag deltas of the step at t and the validity of its samples.  Lane l takes samples
        16l..16l+15; the sample in front of a lane's first is the last of the lane below, and for lane 0 the
        previous step's last (prevX).  Samples behind the chunk read as 0."""
        m = min(STEP, self.n - t)
        xs = np.zeros(STEP, np.int64)
        xs[:m] = self.x[t:t + m]
        valid = np.arange(STEP) < m
        lanes = xs.reshape(64, 16)
        before = np.empty((64, 16), np.int64)
        before[:, 1:] = lanes[:, :-1]
        before[1:, 0] = lanes[:-1, 15]  # the lane below
        before[0, 0] = 0 if (self.fault == "lane0_prev" and self.done) else self.prevX
        self.prevX = int(lanes[63, 15])
        self.done += 1
        before = before.reshape(-1)
        d = (xs - before) & 0xFFFF
        if packed and self.fault == "half_borrow":  # the pair as one 32-bit number: the low half's borrow
            d[1::2] = (d[1::2] - (xs[0::2] < before[0::2])) & 0xFFFF
        return _zz(d), valid, m


class _C5Windows:
    def __init__(self):
        self.S = np.zeros(1088 + 256, np.uint8)
        self.M = np.zeros(1088 + 256, np.uint8)
        self.L = np.zeros(1088, np.uint8)
        self.H = np.zeros(1088, np.uint8)
        self.fS = self.fM = self.fL = 0


def _c5_step(wk, W, t, kind):
    """one step into the windows; returns the 256 key bytes (64 key words)"""
    fault = wk.fault
    z, valid, m = wk.deltas(t, True)
    t1, t2 = (16, 272) if kind == "C5" else (15, 255)
    o1, o2, o3 = (1, 17, 273) if kind == "C5" else (0, 0, 0)
    ge = 1 if fault == "threshold_ge" else 0
    c2, c3 = z > t1 - ge, z > t2 - ge
    cls = (z >= 1).astype(np.int64) + c2 + c3
    if m < STEP and fault != "tail_keys":
        cls[~valid] = 0
    val = (z - (o1 + (o2 - o1) * c2)) & 0xFF if kind == "C5" else z & 0xFF
    cl = cls.reshape(64, 16)
    keys = ((cl << (2 * np.arange(16))).sum(1).astype(np.uint32)).view(np.uint8)  # little-endian key words
    mk = [cl == c for c in (1, 2, 3)]
    cnt = [k.sum(1).astype(np.int64) for k in mk]
    rank = [np.cumsum(k, 1) - k for k in mk]
    pc = cnt[0] | (cnt[1] << 11) | (cnt[2] << 22)
    inc = np.cumsum(pc) & 0xFFFFFFFF
    exc = (inc - pc) & 0xFFFFFFFF
    tot = int(inc[63])
    v2 = val.reshape(64, 16)
    pS = W.fS + (exc & 0x7FF)[:, None] + rank[0]
    pM = W.fM + ((exc >> 11) & 0x7FF)[:, None] + rank[1]
    assert pS[mk[0]].size == 0 or pS[mk[0]].max() < W.S.size
    assert pM[mk[1]].size == 0 or pM[mk[1]].max() < W.M.size
    W.S[pS[mk[0]]] = v2[mk[0]]
    W.M[pM[mk[1]]] = v2[mk[1]]
    # field 3 has 10 bits: the total is rebuilt from the last lane
    t3 = (tot >> 22) if fault == "field3_wrap" else int(exc[63] >> 22) + int(pc[63] >> 22)
    if t3:
        pL = W.fL + (exc >> 22)[:, None] + rank[2]
        w = (z.reshape(64, 16) - o3) & 0xFFFF
        assert pL[mk[2]].size == 0 or pL[mk[2]].max() < W.L.size
        W.L[pL[mk[2]]] = w[mk[2]] & 0xFF
        W.H[pL[mk[2]]] = w[mk[2]] >> 8
    W.fS += tot & 0x7FF
    W.fM += (tot >> 11) & 0x7FF
    W.fL += t3
    return keys


def _pack(W, a, b):
    """window entries [a, b) as bytes: one per entry, or (nibble window) two entries per byte"""
    return W[a:b:2] | (W[a + 1:b:2] << 4)


def _flush(W, fill, out, gpos, nib, fault, fixed=False, lead=None):
    """The complete 16-byte blocks of a window to out + gpos, the tail to the window's front.  fixed: one
    store per lane, lane b stores block min(b, nblk), so the incomplete block goes out too; lead: the first
    block's entries in front of a range's start are not written.  Returns (fill, gpos, lead)."""
    unit = 32 if nib else 16
    nblk, tail = fill // unit, fill % unit
    blocks = list(range(nblk))
    if fixed:
        lanes = 63 if fault == "full_window_63" else 64
        blocks = sorted({min(b, nblk) for b in range(lanes)})
    for b in blocks:
        src = _pack(W, unit * b, unit * b + unit) if nib else W[16 * b:16 * b + 16]
        k0 = 0
        if b == 0 and lead and fault != "lead_written":
            k0 = (lead + 1) >> 1 if nib else lead
            if nib and fault == "odd_lead_byte":
                k0 = lead >> 1
        out[gpos + 16 * b + k0:gpos + 16 * b + 16] = src[k0:]
    if nblk:
        W[:tail] = W[unit * nblk:unit * nblk + tail].copy()
        lead = 0
    elif fault == "carry_dropped":
        tail = 0
    return tail, gpos + 16 * nblk, lead


def _c5_wave(x, n, kind, fault):
    K = np.zeros((n + 3) // 4 + 4 * 64 + 64, np.uint8)
    S = np.zeros(n // 2 + 1 + 64 + 16, np.uint8)
    M, Ll, Lh = (np.zeros(n + 64 + 16, np.uint8) for _ in range(3))
    W, wk = _C5Windows(), _Walk(x, n, fault)
    gS = gM = gL = gH = 0
    fH = 0
    t = 0
    while t + STEP <= n:
        keys = _c5_step(wk, W, t, kind)
        fH = W.fL
        if W.fL >= 16:
            W.fL, gL, _ = _flush(W.L, W.fL, Ll, gL, False, fault)
            fH, gH, _ = _flush(W.H, fH, Lh, gH, False, fault)
        K[t >> 2:(t >> 2) + 256] = keys
        W.fS, gS, _ = _flush(W.S, W.fS, S, gS, True, fault, fixed=True)
        W.fM, gM, _ = _flush(W.M, W.fM, M, gM, False, fault, fixed=True)
        t += STEP
    if t < n:
        keys = _c5_step(wk, W, t, kind)
        nK = (n - t + 3) // 4
        K[t >> 2:(t >> 2) + nK] = keys[:nK]
        W.fS, gS, _ = _flush(W.S, W.fS, S, gS, True, fault)
        W.fM, gM, _ = _flush(W.M, W.fM, M, gM, False, fault)
        fH = W.fL
        W.fL, gL, _ = _flush(W.L, W.fL, Ll, gL, False, fault)
        fH, gH, _ = _flush(W.H, fH, Lh, gH, False, fault)
    fS, fM, fL = W.fS, W.fM, W.fL
    nbS = (fS + 1) // 2
    for j in range(nbS):  # a trailing odd nibble leaves its high half zero
        hi = W.S[2 * j + 1] if (2 * j + 1 < fS or fault == "odd_nibble_high") else 0
        S[gS + j] = W.S[2 * j] | ((int(hi) << 4) & 0xFF)
    M[gM:gM + fM] = W.M[:fM]
    Ll[gL:gL + fL] = W.L[:fL]
    Lh[gH:gH + fL] = W.H[:fL]
    sizes = [(n + 3) // 4, gS + nbS, gM + fM, gL + fL, gL + fL]
    return [b[:s].tobytes() for b, s in zip((K, S, M, Ll, Lh), sizes)]


def _range_counts(x, n, t0, t1):
    """the range's class counts by the scalar class rule (the delta of sample 0 is from 0)"""
    u = x[t0:t1]
    prev = np.concatenate([[x[t0 - 1] if t0 else 0], u[:-1]])
    z = _zz(u - prev)
    return int(((z >= 1) & (z <= 16)).sum()), int(((z > 16) & (z <= 272)).sum()), int((z > 272).sum())


def _c5_ranges(x, n, fault):
    """the 32 single-wave ranges and the last range's walk over the shared S bytes (C5)"""
    K = np.zeros((n + 3) // 4 + 4 * 64 + 64, np.uint8)
    S = np.zeros(n // 2 + 1 + 64 + 16, np.uint8)
    M, Ll, Lh = (np.zeros(n + 64 + 16, np.uint8) for _ in range(3))
    plan = range_plan(n)
    counts = [_range_counts(x, n, t0, t1) if t0 < t1 else (0, 0, 0) for t0, t1 in plan]
    firstNib, lastNib = [0xFF] * RANGES, [0xFF] * RANGES
    late = []  # under odd_lead_byte: the shared bytes a range writes itself, after their owner
    pS = pM = pL = 0
    for r, (t0, t1) in enumerate(plan):
        if t0 < t1:
            W, wk = _C5Windows(), _Walk(x, n, fault)
            W.fS, W.fM, W.fL = pS & 31, pM & 15, pL & 15
            fH = W.fL
            gS, gM, gL = (pS >> 1) & ~15, pM & ~15, pL & ~15
            gH = gL
            leadS, leadM, leadL, leadH = W.fS, W.fM, W.fL, W.fL
            wk.prevX = int(x[t0 - 1]) if (t0 and fault != "range_prev") else 0
            for t in range(t0, t1, STEP):
                keys = _c5_step(wk, W, t, "C5")
                nK = 256 if t + STEP <= n else (n - t + 3) // 4
                K[t >> 2:(t >> 2) + nK] = keys[:nK]
                look = t == t0 or fault != "late_first_entry"
                if firstNib[r] == 0xFF and (pS & 1) and W.fS > leadS and look:
                    firstNib[r] = int(W.S[leadS])
                if fault == "odd_lead_byte" and leadS & 1 and W.fS >= 32:
                    late.append((gS + (leadS >> 1), int(W.S[leadS - 1] | (W.S[leadS] << 4)) & 0xFF))
                fH = W.fL
                W.fS, gS, leadS = _flush(W.S, W.fS, S, gS, True, fault, lead=leadS)
                W.fM, gM, leadM = _flush(W.M, W.fM, M, gM, False, fault, lead=leadM)
                W.fL, gL, leadL = _flush(W.L, W.fL, Ll, gL, False, fault, lead=leadL)
                fH, gH, leadH = _flush(W.H, fH, Lh, gH, False, fault, lead=leadH)
            fS, fM, fL = W.fS, W.fM, W.fL
            for j in range((fS + 1) // 2):  # whole bytes of the range only
                lo_is_lead = 2 * j < leadS
                if fault == "lead_written":
                    lo_is_lead = False
                if fault == "odd_lead_byte" and 2 * j + 1 == leadS and 2 * j + 1 < fS:
                    late.append((gS + j, int(W.S[2 * j] | (W.S[2 * j + 1] << 4)) & 0xFF))
                if lo_is_lead or 2 * j + 1 >= fS:
                    continue
                S[gS + j] = W.S[2 * j] | (W.S[2 * j + 1] << 4)
            if fS > leadS and fS & 1:
                lastNib[r] = int(W.S[fS - 1])
            a = 0 if fault == "lead_written" else leadM
            M[gM + a:gM + fM] = W.M[a:fM]
            a = 0 if fault == "lead_written" else leadL
            Ll[gL + a:gL + fL] = W.L[a:fL]
            Lh[gH + a:gH + fL] = W.H[a:fL]
        cS, cM, cL = counts[r]
        pS, pM, pL = pS + cS, pM + cM, pL + cL
    # the last range: the shared S bytes and a trailing half byte
    at, owner = 0, None
    for v in range(RANGES):
        cv = counts[v][0]
        if fault == "empty_range_owner":
            if at & 1 and v:
                S[at >> 1] = (lastNib[v - 1] | (firstNib[v] << 4)) & 0xFF
            at += cv
            owner = v
            continue
        if cv == 0:
            continue
        if at & 1 and owner is not None:
            S[at >> 1] = (lastNib[owner] | (firstNib[v] << 4)) & 0xFF
        at += cv
        owner = v
    if at & 1 and owner is not None:
        S[at >> 1] = lastNib[RANGES - 1 if fault == "last_half_owner" else owner] & 0xFF
    for pos, b in late:
        S[pos] = b
    sizes = [(n + 3) // 4, (pS + 1) // 2, pM, pL, pL]
    return [b[:s].tobytes() for b, s in zip((K, S, M, Ll, Lh), sizes)]


def _one_bit(x, n, codec, fault):
    """VBZ / C1 (one byte window, 16-bit key words), C2 / C3 (no window: running fills)"""
    if n == 0:
        return [b""] * (1 if codec == "VBZ" else O.VARIANT_FRAMES[codec])
    nk = (n >> 3) + (((n & 7) + 7) >> 3)
    K = np.zeros(nk + 128 + 2, np.uint8)
    wk = _Walk(x, n, fault)
    windowed = codec in ("VBZ", "C1")
    D = np.zeros(3 * n + 64, np.uint8)
    A, B, H = (np.zeros(n + STEP + 32, np.uint8) for _ in range(3))
    Wd = np.zeros(2 * STEP + 32 + 256, np.uint8)
    fill = gpos = fa = fb = 0
    for t in range(0, n, STEP):
        z, valid, m = wk.deltas(t, False)
        if m < STEP and fault == "tail_keys":
            valid = np.ones(STEP, bool)
        big = valid & (z > 255)
        kb = np.packbits(big, bitorder="little")
        k0 = t >> 3
        cnt = min(128, nk - k0)
        K[k0:k0 + cnt] = kb[:cnt]
        lo, hi = (z & 0xFF).astype(np.uint8), (z >> 8).astype(np.uint8)
        if windowed:
            w = valid.astype(np.int64) + big
            pos = fill + np.cumsum(w) - w
            Wd[pos[valid]] = lo[valid]
            Wd[pos[big] + 1] = hi[big]
            fill += int(w.sum())
            fill, gpos, _ = _flush(Wd, fill, D, gpos, False, fault)
        elif codec == "C2":
            A[t:t + int(valid.sum())] = lo[valid]
            H[fb:fb + int(big.sum())] = hi[big]
            fb += int(big.sum())
        else:
            small = valid & ~big
            A[fa:fa + int(small.sum())] = lo[small]
            B[fb:fb + int(big.sum())] = lo[big]
            H[fb:fb + int(big.sum())] = hi[big]
            fa += int(small.sum())
            fb += int(big.sum())
    if windowed:
        D[gpos:gpos + fill] = Wd[:fill]
        data = D[:gpos + fill].tobytes()
        keys = K[:nk].tobytes()
        return [keys + data] if codec == "VBZ" else [keys, data]
    if codec == "C2":
        return [K[:nk].tobytes(), A[:n].tobytes(), H[:fb].tobytes()]
    return [K[:nk].tobytes(), A[:fa].tobytes(), B[:fb].tobytes(), H[:fb].tobytes()]


def _vbz0(x, n, fault):
    nk = (n + 3) // 4
    K = np.zeros(nk + 256 + 4, np.uint8)
    D = np.zeros(2 * n + 64 + 16, np.uint8)
    N = np.zeros(4 * STEP + 64, np.uint8)
    wk = _Walk(x, n, fault)
    fill = gpos = 0
    for t in range(0, n, STEP):
        z, valid, m = wk.deltas(t, False)
        cls = (z >= 1).astype(np.int64) + (z > 16) + (z > 272)
        if m < STEP and fault != "tail_keys":
            cls[~valid] = 0
        keys = ((cls.reshape(64, 16) << (2 * np.arange(16))).sum(1).astype(np.uint32)).view(np.uint8)
        nK = 256 if m == STEP else (n - t + 3) // 4
        K[t >> 2:(t >> 2) + nK] = keys[:nK]
        k = np.where(cls == 3, 4, cls)
        w = (z - np.choose(cls, [0, 1, 17, 273])) & 0xFFFF
        pos = fill + np.cumsum(k) - k
        for j in range(4):
            sel = k > j
            N[pos[sel] + j] = (w[sel] >> (4 * j)) & 15
        fill += int(k.sum())
        fill, gpos, _ = _flush(N, fill, D, gpos, True, fault)
    if n == 0:
        return [b""]
    nb = (fill + 1) // 2
    for j in range(nb):
        hi = N[2 * j + 1] if (2 * j + 1 < fill or fault == "odd_nibble_high") else 0
        D[gpos + j] = N[2 * j] | ((int(hi) << 4) & 0xFF)
    return [K[:nk].tobytes() + D[:gpos + nb].tobytes()]


def split_as_device(x, codec, ranges=False, fault=None):
    """The streams of one chunk by a restatement of the device split: steps of 1,024, lanes of 16, the delta
    from the lane below and the previous step, the packed prefix (11, 11, 10 bits) with the class-3 total
    rebuilt from the last lane, windows with a carried tail and block-wise output; with `ranges` (C5) the 32
    ranges with their leads, x[t0 - 1] and the shared-byte walk.  `fault`: one name of FAULTS."""
    assert fault is None or fault in FAULTS
    u = np.asarray(x, np.int16).view(np.uint16).astype(np.int64)
    n = u.size
    if codec in FIVE:
        if ranges:
            assert codec == "C5"
            return _c5_ranges(u, n, fault)
        return _c5_wave(u, n, "C5" if codec == "C5" else "C4", fault)
    if codec == "VBZ0":
        return _vbz0(u, n, fault)
    return _one_bit(u, n, codec, fault)


# ---- the catalogue -------------------------------------------------------------------------------------------
def _perm(count, total=STEP, mult=389):
    """`count` scattered places of a step (389 is odd: i -> 389 i mod 1,024 is a permutation)"""
    return (np.arange(count) * mult) % total


def _mixed(nsamp, seed):
    """uniformly mixed classes, another pattern for every seed"""
    i = np.arange(nsamp)
    return ((i * 7 + seed) ^ (i >> 3) ^ (seed * 5)) % 4


def _step_of(counts, fillcls=0, seed=0):
    """one full step holding counts[c] samples of class c at scattered places, the rest of class fillcls"""
    cls = np.full(STEP, fillcls, np.int64)
    places = _perm(STEP, mult=389 + 2 * seed)
    p = 0
    for c, k in counts.items():
        cls[places[p:p + k]] = c
        p += k
    assert p <= STEP
    return cls


def _placed(c, a, b, place):
    """one full step with exactly c samples of class a, the rest of class b"""
    cls = np.full(STEP, b, np.int64)
    if place == "low":
        cls[:c] = a
    elif place == "high":
        cls[STEP - c:] = a
    else:  # one per lane: the fewer of the two classes, lane i's sample i % 16
        few, k, other = (a, c, b) if c <= 512 else (b, STEP - c, a)
        cls[:] = other
        lanes = np.arange(min(k, 64))
        cls[16 * lanes + lanes % 16] = few
        cls[np.flatnonzero(cls == other)[: k - lanes.size]] = few  # beyond 64: the first remaining ones
    assert int((cls == a).sum()) == c
    return cls


def _case(name, cls, codecs=None, claims=None, kind="C5"):
    cls = np.concatenate([np.asarray(c, np.int64) for c in cls]) if isinstance(cls, list) else np.asarray(cls)
    return Case(name, signal(coded(cls, kind)), codecs, claims)


def _values():
    out = []
    base = coded(_mixed(1040, 3) % 2)  # classes 0 and 1 around the marks
    for n, first, tag in ((1024, 0, "first_zero"), (1040, 65535, "first_min"), (1040, 65534, "first_max")):
        z = base[:n].copy()
        for i, v in enumerate(THRESHOLDS):
            z[32 + 6 * i] = v   # an even sample: the low half of a packed word
            z[35 + 6 * i] = v   # an odd one: the high half
        if n > STEP:
            for i, v in enumerate((16, 17, 272, 273, 255, 256, 15)):
                z[STEP + 2 * i + (i & 1)] = v
        z[0] = first
        x = signal(z)
        want = {0: 0, 65535: -32768, 65534: 32767}[first]
        assert int(x[0]) == want
        out.append(Case(f"values/thresholds_{n}_{tag}", x, claims={
            f"{n} samples": ("C5", lambda sh, n=n: sh["n"] == n),
            "C5 sees all four classes": ("C5", lambda sh: set(sh["classes"]) == {0, 1, 2, 3}),
            "C4 sees all four classes": ("C4", lambda sh: set(sh["classes"]) == {0, 1, 2, 3}),
            "the 1-bit codecs see both": ("C1", lambda sh: set(sh["classes"]) == {0, 1})}))
    z = base[:STEP].copy()
    for i in range(12):  # a borrow between the halves of a pair, and none
        z[16 + 8 * i], z[17 + 8 * i] = (65535, 0) if i & 1 else (0, 65535)
    out.append(Case("values/borrow_pairs_1024", signal(z)))
    x = signal(base[:1040]).copy()
    x[100:108] = [32767, -32768, 32767, -32768, 0, -32768, -32768, 32767]  # deltas that wrap int16
    x[1025:1029] = [32767, -32768, 0, -32768]
    out.append(Case("values/int16_wrap_1040", x, claims={
        "-32768 -> 0 is zig-zag 65535, class 3": ("C5", lambda sh: zigzag_of(x)[104] == 65535 and sh["classes"][104] == 3),
        "32767 -> -32768 is zig-zag 2, class 1": ("C5", lambda sh: zigzag_of(x)[101] == 2 and sh["classes"][101] == 1)}))
    return out


def _seams():
    out = []
    marks = [16 * l for l in (1, 31, 32, 63)] + [STEP, 2 * STEP, 3 * STEP]
    n = 3 * STEP + 40
    for tag, bg, mk in (("large_among_small", 1, 3), ("small_among_large", 3, 1)):
        cls = np.full(n, bg, np.int64)
        cls[marks] = mk
        out.append(_case(f"seams/{tag}_{n}", cls, claims={
            "the marks stand at lane and step seams": (
                "C5", lambda sh, mk=mk: [int(i) for i in np.flatnonzero(sh["classes"] == mk)] == marks),
            "the last step is ragged and starts with a mark": ("C5", lambda sh: not sh["steps"][3]["full"])}))
        n33 = 33 * STEP
        plan = range_plan(n33)
        at = [plan[r][0] for r in (1, 2, 16, 31)]
        cls = np.full(n33, bg, np.int64)
        if bg == 3:  # class 3 in the steps around the marks only: 33 steps of it do not fit C1's capacity
            cls[:] = 2
            for a in at:
                cls[a - STEP:a + STEP] = 3
        cls[at] = mk
        out.append(_case(f"seams/ranges_33_{tag}", cls, claims={
            "the marks are the first samples of ranges 1, 2, 16 and 31": (
                "C5", lambda sh, mk=mk, at=at: [int(i) for i in np.flatnonzero(sh["classes"] == mk)] == at
                and [sh["ranges"][r]["t0"] for r in (1, 2, 16, 31)] == at),
            "range 31 holds two steps": ("C5", lambda sh: sh["ranges"][31]["steps"] == 2)}))
    return out


COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 1008, 1023, 1024]
PAIRS = [(1, 0), (2, 0), (3, 0), (1, 2), (1, 3), (2, 3)]


def _counts():
    """[c of a at the lowest lanes, mixed, c of a at the highest lanes, mixed, one per lane, mixed, ragged]"""
    out = []
    for a, b in PAIRS:
        for c in COUNTS:
            cls = []
            for j, place in enumerate(("low", "high", "lane")):
                cls += [_placed(c, a, b, place), _mixed(STEP, 11 * j + c + a)]
            cls.append(_mixed(37, c))
            key = {1: "n1", 2: "n2", 3: "n3"}[a]
            claims = {f"steps 0, 2 and 4 hold exactly {c} samples of class {a}": (
                "C5", lambda sh, key=key, c=c: [sh["steps"][j][key] for j in (0, 2, 4)] == [c, c, c])}
            if (a, c) == (3, 1024):
                claims["steps 0, 2 and 4 wrap the third field"] = (
                    "C5", lambda sh: all(sh["steps"][j]["field3_wraps"] for j in (0, 2, 4)))
                claims["and for C4"] = ("C4", lambda sh: all(sh["steps"][j]["field3_wraps"] for j in (0, 2, 4)))
            if (a, b, c) == (3, 0, 1023):
                claims["the odd one is sample 1,023 and then sample 0"] = (
                    "C5", lambda sh: sh["classes"][1023] == 0 and sh["classes"][2 * STEP] == 0)
            if (a, c) == (2, 1024):
                claims["M leaves 64 blocks or more in one step"] = ("C5", lambda sh: sh["steps"][0]["M"]["blocks"] >= 64)
            out.append(_case(f"counts/class{a}_in_{b}_x{c}", cls, claims=claims))
    # C4's own thresholds: its class 2 ends at 255 and its class 3 starts at 256
    for a in (1, 2, 3):
        for c in (1023, 1024):
            cls = []
            for j, place in enumerate(("low", "high", "lane")):
                cls += [_placed(c, a, 0, place), _mixed(STEP, 7 * j + c + a)]
            cls.append(_mixed(37, c + 1))
            key = {1: "n1", 2: "n2", 3: "n3"}[a]
            claims = {f"steps 0, 2 and 4 hold exactly {c} samples of C4's class {a}": (
                "C4", lambda sh, key=key, c=c: [sh["steps"][j][key] for j in (0, 2, 4)] == [c, c, c])}
            if (a, c) == (2, 1024):
                claims["M leaves 64 blocks in one step"] = ("C4", lambda sh: sh["steps"][0]["M"]["blocks"] >= 64)
            out.append(_case(f"counts/c4_class{a}_in_0_x{c}", cls, claims=claims, kind="C4"))
    return out


def _carries():
    out = []
    fills = [(0, 0, 15), (1, 1, 16), (30, 15, 17), (31, 15, 16)]

    def amount(kind, fill, unit):
        return {"none": 0, "one": 1, "to_end": unit - fill if fill else unit, "past_end": (unit - fill if fill else unit) + 1}[kind]

    for fS, fM, fL in fills:
        first = _step_of({1: 64 + fS, 2: 32 + fM, 3: fL}, seed=fS)
        rL = fL % 16
        plans = [(k, {1: amount(k, fS, 32), 2: amount(k, fM, 16), 3: amount(k, rL, 16)})
                 for k in ("none", "one", "to_end", "past_end")]
        plans += [(f"all_class{c}", {c: STEP}) for c in (1, 2, 3)]
        for tag, add in plans:
            cls = [first, _step_of(add, seed=3), _mixed(STEP, fS + 1), _mixed(21, fM)]
            claims = {
                f"step 1 enters with S fill {fS}": ("C5", lambda sh, v=fS: sh["steps"][1]["S"]["before"] == v),
                f"step 1 enters with M fill {fM}": ("C5", lambda sh, v=fM: sh["steps"][1]["M"]["before"] == v),
                f"step 1 enters with class-3 fill {rL}": ("C5", lambda sh, v=rL: sh["steps"][1]["L"]["before"] == v),
                f"step 0 reaches class-3 fill {fL}": ("C5", lambda sh, v=fL: sh["steps"][0]["L"]["fill"] == v),
                "step 1 adds what it says": ("C5", lambda sh, add=add: all(
                    sh["steps"][1][k] == add.get(c, 0) for c, k in ((1, "n1"), (2, "n2"), (3, "n3")))),
            }
            if tag == "all_class1" and fS == 31:
                claims["the S window holds 1,055 nibbles"] = ("C5", lambda sh: sh["steps"][1]["S"]["fill"] == 1055)
            if tag == "all_class2" and fM == 15:
                claims["the M window holds 1,039 bytes"] = ("C5", lambda sh: sh["steps"][1]["M"]["fill"] == 1039)
            if tag == "all_class3" and fL == 15:
                claims["the class-3 window holds 1,039 bytes"] = ("C5", lambda sh: sh["steps"][1]["L"]["fill"] == 1039)
            if tag == "to_end":
                claims["S ends on a block end"] = ("C5", lambda sh: sh["steps"][1]["S"]["after"] == 0)
                claims["M ends on a block end"] = ("C5", lambda sh: sh["steps"][1]["M"]["after"] == 0)
            out.append(_case(f"carries/S{fS}_M{fM}_L{fL}_{tag}", cls, claims=claims))
    # a stream that gets nothing for three steps while it holds a carry, then gets more
    for c in (1, 2, 3):
        quiet = [np.where(_mixed(STEP, 5 + j) == c, 0, _mixed(STEP, 5 + j)) for j in range(3)]
        cls = [_step_of({1: 37, 2: 19, 3: 5}, seed=c)] + quiet + [_mixed(STEP, 9), _mixed(45, 2)]
        key, win = {1: ("n1", "S"), 2: ("n2", "M"), 3: ("n3", "L")}[c]
        out.append(_case(f"carries/starved_class{c}", cls, claims={
            f"steps 1 to 3 add nothing to {win}, which holds a carry": (
                "C5", lambda sh, key=key, win=win: all(sh["steps"][j][key] == 0 and sh["steps"][j][win]["before"] > 0
                                                       and sh["steps"][j][win]["blocks"] == 0 for j in (1, 2, 3))),
            "step 4 adds more": ("C5", lambda sh, key=key: sh["steps"][4][key] > 0)}))
    cls = [_step_of({1: 100, 2: 50, 3: 4}), _step_of({1: 60, 2: 70, 3: 5}, seed=1), _step_of({3: 3, 1: 9}, seed=2)[:300]]
    out.append(_case("carries/class3_tail_only", cls, claims={
        "the class-3 fill never reaches 16": ("C5", lambda sh: max(s["L"]["fill"] for s in sh["steps"]) < 16
                                              and 0 < sh["totals"][2] < 16)}))
    # the byte-wide window of VBZ / C1: a step leaves 1,024 + big bytes
    for r in (0, 1, 15):
        for tag, big in (("small_only", 0), ("to_end", (16 - r) % 16), ("past_end", (16 - r) % 16 + 1), ("all_big", STEP)):
            cls = [_step_of({3: r + 16}, fillcls=1, seed=r), _step_of({3: big}, fillcls=1, seed=2), _mixed(STEP, r),
                   _mixed(29, r)]
            claims = {f"step 1 enters with {r} carried bytes": ("VBZ", lambda sh, r=r: sh["steps"][1]["D"]["before"] == r),
                      f"step 1 has {big} big samples": ("C1", lambda sh, big=big: sh["steps"][1]["big"] == big)}
            if tag == "all_big" and r == 15:
                claims["the window holds 15 + 2,048 bytes"] = ("VBZ", lambda sh: sh["steps"][1]["D"]["fill"] == 2063)
            if tag == "to_end":
                claims["the step ends on a block end"] = ("VBZ", lambda sh: sh["steps"][1]["D"]["after"] == 0)
            out.append(_case(f"carries/bytes_{r}_{tag}", cls, codecs=ONE_BIT, claims=claims))
    for carried in (31, 1):
        cls = [_step_of({1: carried}), np.full(STEP, 3), _mixed(STEP, 4), _mixed(33, 1)]
        out.append(_case(f"carries/vbz0_{carried}_plus_4096", cls, codecs=("VBZ0", "C5", "C4"), claims={
            f"{carried} carried nibbles plus 4,096": ("VBZ0", lambda sh, v=carried: sh["steps"][1]["N"]["before"] == v
                                                     and sh["steps"][1]["N"]["fill"] == v + 4096)}))
    return out


RAGGED_R = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1007, 1008, 1009, 1023]


def _ragged():
    out = []
    for k in (0, 1, 2):
        for i, r in enumerate(RAGGED_R):
            n = STEP * k + r
            cls = _mixed(n, 13 * k + i)
            if (i + k) % 6 == 5:
                cls = np.where(cls == 1, 2, cls)  # a nibble total of none
            cls[n - 1] = 3 if i % 3 else 2        # the last sample is far from 0's neighbourhood
            claims = {f"{k} full steps and {r} samples": (
                "C5", lambda sh, k=k, r=r: len(sh["steps"]) == k + 1 and sh["steps"][-1]["samples"] == r
                and not sh["steps"][-1]["full"])}
            if (i + k) % 6 == 5:
                claims["no nibble at all"] = ("C5", lambda sh: sh["totals"][0] == 0)
            out.append(_case(f"ragged/{k}x1024_plus_{r}", cls, claims=claims))
    return out


def _by_ranges(steps, fn, last=None):
    """a chunk of `steps` steps (the last one `last` samples long) from fn(r, samples of range r) -> classes"""
    n = steps * STEP if last is None else (steps - 1) * STEP + last
    cls = np.zeros(n, np.int64)
    for r, (t0, t1) in enumerate(range_plan(n)):
        if t0 < t1:
            c = np.asarray(fn(r, t1 - t0), np.int64)
            assert c.size == t1 - t0
            cls[t0:t1] = c
    return cls


def _range_of(m, counts, seed):
    """m samples with counts[c] samples of class c at scattered places of the range's first step"""
    cls = np.zeros(m, np.int64)
    cls[: min(m, STEP)] = _step_of(counts, seed=seed)[: min(m, STEP)]
    return cls


def _ranges():
    out = []

    def nonempty(sh):
        return [g for g in sh["ranges"] if not g["empty"]]

    for steps in (1, 2, 31, 32, 33, 47, 64, 256):
        last = 1000 if steps in (1, 33, 47) else None
        cls = _by_ranges(steps, lambda r, m: _range_of(m, {1: 1 + 2 * (r % 7), 2: 3 + r % 5, 3: r % 4}, r), last)
        out.append(_case(f"ranges/odd_class1_every_range_{steps}_steps", cls, claims={
            "every range with samples holds an odd number of class 1": (
                "C5", lambda sh: all(g["cS"] & 1 for g in nonempty(sh))),
            f"{min(steps, 32)} ranges hold samples": ("C5", lambda sh, k=min(steps, 32): len(nonempty(sh)) == k)}))

    def between(r, m):
        if r in (7, 12, 13):
            return _range_of(m, {2: 40, 3: 9}, r)
        return _range_of(m, {1: 5 if r in (6, 9, 11) else 6 + 2 * (r % 3), 2: 7, 3: 2}, r)

    out.append(_case("ranges/no_class1_between_odd_neighbours_32_steps", _by_ranges(32, between), claims={
        "range 7 holds no class 1, ranges 6 and 8 meet on an odd nibble": (
            "C5", lambda sh: not sh["ranges"][7]["nibbles"] and sh["ranges"][8]["pS"] & 1
            and (sh["ranges"][8]["pS"] >> 1) in sh["shared"] and sh["shared"][sh["ranges"][8]["pS"] >> 1] == (6, 8)),
        "ranges 12 and 13 hold none, 11 and 14 share a byte": (
            "C5", lambda sh: not sh["ranges"][12]["nibbles"] and not sh["ranges"][13]["nibbles"]
            and sh["shared"].get(sh["ranges"][14]["pS"] >> 1) == (11, 14))}))
    for steps in (32, 47):
        cls = _by_ranges(steps, lambda r, m: _range_of(m, {1: 0 if r < 5 else 3 + 2 * (r % 4), 2: 11, 3: 3}, r))
        out.append(_case(f"ranges/no_class1_in_the_first_ranges_{steps}_steps", cls, claims={
            "ranges 0 to 4 hold no class 1": ("C5", lambda sh: not any(sh["ranges"][r]["nibbles"] for r in range(5)))}))
    for steps in (32, 33):
        cls = _by_ranges(steps, lambda r, m: _range_of(m, {1: 0 if r >= 27 else (3 if r == 26 else 4), 2: 9, 3: 1}, r))
        out.append(_case(f"ranges/no_class1_in_the_last_ranges_{steps}_steps", cls, claims={
            "ranges 27 to 31 hold no class 1 and the total is odd": (
                "C5", lambda sh: not any(sh["ranges"][r]["nibbles"] for r in range(27, 32)) and sh["totals"][0] & 1),
            "the trailing half byte is range 26's": ("C5", lambda sh: sh["trailing_owner"] == 26)}))
    # range starts inside a block: ranges 2j set the offsets, ranges 2j + 1 start there and add a chosen amount
    s_combo = [(o, a) for o in (1, 2, 30, 31) for a in ("none", "one", "to_end", "past_end", "many")]
    b_combo = [(o, a) for o in (1, 15) for a in ("none", "one", "to_end", "past_end", "many")]

    def add_of(kind, off, unit):
        return {"none": 0, "one": 1, "to_end": unit - off, "past_end": unit - off + 1, "many": 300}[kind]

    for part in (0, 1):
        targets, pos = {}, [0, 0, 0]
        per_range = {}
        for j in range(16):
            i = 16 * part + j
            (oS, aS), (oM, aM), (oL, aL) = s_combo[i % 20], b_combo[i % 10], b_combo[(i + 3) % 10]
            setter = {1: (oS - pos[0]) % 32 + 32, 2: (oM - pos[1]) % 16 + 16, 3: (oL - pos[2]) % 16 + 16}
            target = {1: add_of(aS, oS, 32), 2: add_of(aM, oM, 16), 3: add_of(aL, oL, 16)}
            per_range[2 * j], per_range[2 * j + 1] = setter, target
            targets[2 * j + 1] = (oS, oM, oL, target)
            for k, c in enumerate((1, 2, 3)):
                pos[k] += setter[c] + target[c]
        cls = _by_ranges(32, lambda r, m: _range_of(m, per_range[r], r))
        out.append(_case(f"ranges/starts_inside_a_block_{part}", cls, claims={
            "the odd ranges start at the chosen offsets and add the chosen amounts": (
                "C5", lambda sh, targets=targets: all(
                    (sh["ranges"][r]["pS"] % 32, sh["ranges"][r]["pM"] % 16, sh["ranges"][r]["pL"] % 16) == (oS, oM, oL)
                    and (sh["ranges"][r]["cS"], sh["ranges"][r]["cM"], sh["ranges"][r]["cL"]) == (t[1], t[2], t[3])
                    for r, (oS, oM, oL, t) in targets.items()))}))

    def late(r, m):  # ranges of two steps: the first class-1 sample of ranges 3 and 9 in their second step
        cls = np.zeros(m, np.int64)
        if r in (3, 9):
            cls[:STEP] = _step_of({2: 20, 3: 3}, seed=r)
            cls[STEP:] = _step_of({1: 8, 2: 5}, seed=r + 1)
        else:
            cls[:STEP] = _step_of({1: 5 if r == 2 else 4, 2: 6, 3: 1}, seed=r)
            cls[STEP:] = _step_of({1: 2, 2: 3}, seed=r + 2)
        return cls

    out.append(_case("ranges/first_entry_in_the_second_step_64_steps", _by_ranges(64, late), claims={
        "ranges 3 and 9 start on an odd nibble and find their first in their second step": (
            "C5", lambda sh: all(sh["ranges"][r]["pS"] & 1 and sh["ranges"][r]["first_nibble_step"] == 1
                                 and sh["ranges"][r]["steps"] == 2 for r in (3, 9)))}))
    return out


def _capacity():
    out = []
    for c in (1, 2, 3):
        out.append(_case(f"capacity/all_class{c}_262144", np.full(PASS_SAMPLES, c), claims={
            f"every sample is class {c}": ("C5", lambda sh, c=c: sh["totals"][c - 1] == PASS_SAMPLES)}))
    n = PASS_SAMPLES + 1031
    out.append(_case(f"capacity/mixed_{n}", _mixed(n, 6), claims={
        "above one pass's chunk size": ("C5", lambda sh: sh["n"] > PASS_SAMPLES)}))
    return out


_CAT = None


def catalogue():
    global _CAT
    if _CAT is None:
        _CAT = _values() + _seams() + _counts() + _carries() + _ragged() + _ranges() + _capacity()
        names = [c.name for c in _CAT]
        assert len(set(names)) == len(names)
    return _CAT


def cases(family=None, codec=None, max_n=None, min_n=0):
    return [c for c in catalogue() if (family is None or c.family == family) and (codec is None or codec in c.codecs)
            and (max_n is None or c.n <= max_n) and c.n >= min_n]


def locate(x, codec, stream, byte):
    """Where byte `byte` of stream `stream` of a chunk comes from, for failure messages: (sample, step, range)
    of the first sample that writes into it, by the oracle's classes; range is None but for C5.  None where the
    byte lies behind the stream or the codec keeps no such stream apart (VBZ0, VBZ: the one frame)."""
    if codec not in FIVE:
        return None
    cls = oracle_classes(x, codec)
    if stream == 0:
        i = 4 * byte
    else:
        idx = np.flatnonzero(cls == min(stream, 3))
        k = 2 * byte if stream == 1 else byte
        if k >= idx.size:
            return None
        i = int(idx[k])
    if i >= cls.size:
        return None
    rng = None
    if codec == "C5":
        rng = next(r for r, (t0, t1) in enumerate(range_plan(cls.size)) if t0 <= i < t1)
    return i, i // STEP, rng
