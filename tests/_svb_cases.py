"""Stream sets that no split writes, for the merge half of every decoder (tests only, CPU only).

A split always writes exactly ceil(n/4) or svb16_key_length(n) key bytes, zero bits in the unused codes
of the last key byte, a zero high nibble after an odd nibble count, and streams exactly as long as the
keys demand.  The reference's decoders require none of it: they walk the decoded streams as one
concatenated buffer whose starts are the key length of n, then + the middle frames' decoded sizes; the
keys frame's own size is never used and the last frame's size only enters the total; a short stream
reads on into the next one; the status comes from a read past the buffer (CORRUPT here, undefined
behaviour there) and from `consumed != total` ("Remaining data").

catalogue() builds named cases for the seven codecs.  Every frame of every blob is libzstd's own
level-1 frame of the case's raw bytes (O.zstd_compress1), joined with O.variant_assemble (VBZ0 and VBZ:
the one frame alone), so nothing here touches the zstd layer.  `rc` and `want` are the oracle's
(O.variant_decompress / O.vbz_decompress), `designed` the status the recipe was built for
(tests/test_svb_cases.py holds the two together), `claims` the documented rule by which a chunk leaves
the staged passes for the claims pass (a frame's content above n bytes, or the contents + 16 above
2.25 n + 1,024).

Families: A exact, B tail, C recut, D borrow, E remaining, F corrupt, G empty, H vbz_pad.
"""
from __future__ import annotations

import zlib

import numpy as np

import _oracle as O

CODECS = ["C5", "C4", "C1", "C2", "C3", "VBZ0", "VBZ"]
TWO_BIT = ("C5", "C4", "VBZ0")
ONE_FRAME = ("VBZ0", "VBZ")
FIVE = ("C5", "C4")
FAMILIES = ["exact", "tail", "recut", "borrow", "remaining", "corrupt", "empty", "vbz_pad"]
# which codecs a family has recipes for
APPLIES = {
    "exact": CODECS, "tail": CODECS, "recut": ["C5", "C4", "C1", "C2", "C3"], "borrow": CODECS,
    "remaining": CODECS, "corrupt": ["C5", "C4", "C1", "C2", "C3", "VBZ0"], "empty": CODECS,
    "vbz_pad": ["VBZ", "VBZ0"],
}
SMALL_SIZES = [1, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 2057, 40967]
BIG_SIZES = [262144, 263173]
CORE_SIZES = [5, 1025, 40967]
VBZ_PADDING = 16

# zigzag value ranges of the classes, and the exact thresholds
_CLASSES = {
    "C5": [(0, 0), (1, 16), (17, 272), (273, 65535)],
    "C4": [(0, 0), (1, 15), (16, 255), (256, 65535)],
    "one": [(0, 255), (256, 65535)],
}
_THRESHOLDS = {
    "C5": [0, 1, 16, 17, 272, 273, 65535],
    "C4": [0, 1, 15, 16, 255, 256, 65535],
    "one": [0, 255, 256, 65535],
}


def class_kind(codec):
    return "C4" if codec == "C4" else ("C5" if codec in ("C5", "VBZ0") else "one")


def key_len(codec, n):
    return (n + 3) // 4 if codec in TWO_BIT else (n >> 3) + (((n & 7) + 7) >> 3)


def mixes(codec):
    k = len(_CLASSES[class_kind(codec)])
    return ["uniform"] + [f"only{c}" for c in range(k)] + ["thresholds"]


class Case:
    def __init__(self, name, family, codec, n, frames, designed, signal=None):
        self.name, self.family, self.codec, self.n = name, family, codec, n
        self.designed, self.signal = designed, signal
        self.frames = [bytes(f) for f in frames]  # the raw content of every zstd frame
        z = [O.zstd_compress1(f) for f in self.frames]
        self.blob = z[0] if codec in ONE_FRAME else O.variant_assemble(z)
        if codec == "VBZ":
            self.rc, self.want = O.vbz_decompress(self.blob, n)
        else:
            self.rc, self.want = O.variant_decompress(codec, self.blob, n)
        sizes = [len(f) for f in self.frames]
        self.claims = max(sizes) > n or sum(sizes) + VBZ_PADDING > n * 9 // 4 + 1024

    @property
    def inter(self):
        return b"".join(self.frames)

    @property
    def d(self):
        return [len(f) for f in self.frames]

    def __iter__(self):  # (name, family, codec, n, blob, rc, want, claims)
        return iter((self.name, self.family, self.codec, self.n, self.blob, self.rc, self.want, self.claims))

    def __repr__(self):
        return f"Case({self.name})"


# ---- signals ------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def draw_classes(rng, codec, n, mix):
    k = len(_CLASSES[class_kind(codec)])
    if mix == "uniform":
        return rng.integers(0, k, n)
    if mix == "light":  # few bytes per sample: the blob stays below the claims rule
        return rng.choice(k, size=n, p=[0.45, 0.4, 0.1, 0.05] if k == 4 else [1.0, 0.0])
    if mix.startswith("only"):
        return np.full(n, int(mix[4:]), np.int64)
    raise ValueError(mix)


def draw_values(rng, codec, n, mix, last_big=False):
    """n zigzag values in the chosen class mix"""
    kind = class_kind(codec)
    if mix == "thresholds":
        t = _THRESHOLDS[kind]
        v = np.array((t * (n // len(t) + 1))[:n], np.int64)
    else:
        cls = draw_classes(rng, codec, n, mix)
        lo = np.array([a for a, _ in _CLASSES[kind]])[cls]
        hi = np.array([b for _, b in _CLASSES[kind]])[cls]
        v = lo + (rng.integers(0, 1 << 30, n) % (hi - lo + 1))
    if last_big and n:
        v[-1] = 40000
    return v


def signal_of(v):
    d = (v >> 1) ^ -(v & 1)
    return (np.cumsum(d) & 0xFFFF).astype(np.uint16).view(np.int16)


def parts_of(codec, x):
    """The split's own streams: one per frame, for VBZ0 / VBZ the keys and the data of the one buffer."""
    n = x.size
    if codec == "VBZ":
        buf = O.oracle_vbz_svb_encode(x)
    elif codec == "VBZ0":
        (buf,) = O.variant_streams(codec, x)
    else:
        return O.variant_streams(codec, x)
    kl = key_len(codec, n)
    return [buf[:kl], buf[kl:]]


def frames_of(codec, parts):
    return [b"".join(parts)] if codec in ONE_FRAME else list(parts)


def pack_keys(codec, classes):
    c = np.asarray(classes, np.uint8)
    per, bits = (4, 2) if codec in TWO_BIT else (8, 1)
    c = np.concatenate([c, np.zeros((-c.size) % per, np.uint8)]).reshape(-1, per).astype(np.uint32)
    return (c << (bits * np.arange(per, dtype=np.uint32))).sum(axis=1).astype(np.uint8).tobytes()


def _rb(rng, n):
    return rng.integers(0, 256, max(int(n), 0), dtype=np.uint8).tobytes()


# ---- families -----------------------------------------------------------------------------------------
def _exact(out):
    for codec in CODECS:
        for n in SMALL_SIZES + BIG_SIZES:
            for mix in (mixes(codec) if n in SMALL_SIZES else ["uniform"]):
                x = signal_of(draw_values(_rng("A", codec, n, mix), codec, n, mix))
                out.append(Case(f"A_{codec}_{n}_{mix}", "exact", codec, n, frames_of(codec, parts_of(codec, x)), 0, x))


def _tail(out):
    for codec in CODECS:
        per = 4 if codec in TWO_BIT else 8
        for n in SMALL_SIZES:
            if n % per == 0:
                continue
            for mix in ("uniform", "only0", "only1") + (("only3",) if codec in TWO_BIT else ()):
                if mix == "uniform" and n not in CORE_SIZES:
                    continue
                x = signal_of(draw_values(_rng("B", codec, n, mix), codec, n, mix))
                parts = [bytearray(p) for p in parts_of(codec, x)]
                used = n % per
                for pat in ((1, 2, 3) if codec in TWO_BIT else (1,)):
                    p = [bytearray(q) for q in parts]
                    if codec in TWO_BIT:
                        fill = (pat * 0x55) & 0xFF & ~((1 << (2 * used)) - 1)
                    else:
                        fill = 0xFF & ~((1 << used) - 1)
                    p[0][-1] |= fill
                    # an odd nibble count leaves the high nibble of the last S (VBZ0: data) byte unused
                    if codec in TWO_BIT:
                        keys = np.frombuffer(bytes(parts[0]), np.uint8)
                        codes = ((keys[:, None] >> (2 * np.arange(4))) & 3).reshape(-1)[:n]
                        nib = int((codes == 1).sum()) if codec in FIVE else int(
                            (codes == 1).sum() + 2 * (codes == 2).sum() + 4 * (codes == 3).sum())
                        if nib & 1:
                            assert p[1][-1] >> 4 == 0
                            p[1][-1] |= 0xF0
                    out.append(Case(f"B_{codec}_{n}_{mix}_pat{pat}", "tail", codec, n, frames_of(codec, p), 0, x))


def _recut(out):
    for codec in APPLIES["recut"]:
        for n in CORE_SIZES:
            for mix in ("uniform", "light"):
                x = signal_of(draw_values(_rng("C", codec, n, mix), codec, n, mix))
                parts = parts_of(codec, x)
                buf, kl, mid = b"".join(parts), len(parts[0]), [len(p) for p in parts[1:-1]]
                for tag, dk in (("0", 0), ("klm1", kl - 1), ("klp1", kl + 1), ("klpd1", kl + len(parts[1]))):
                    if dk < 0 or dk + sum(mid) > len(buf):
                        continue  # the buffer is too short for this cut
                    cuts = np.cumsum([0, dk] + mid).tolist() + [len(buf)]
                    frames = [buf[cuts[i]:cuts[i + 1]] for i in range(len(parts))]
                    out.append(Case(f"C_{codec}_{n}_{mix}_dK{tag}", "recut", codec, n, frames, 0, x))


def _borrow_sizes(codec, cnt):
    """name -> middle sizes and the last size of hand-made stream sets whose walks all stay inside the
    buffer and whose last stream holds exactly the big-class count (cnt: the class counts)"""
    if codec in FIVE:
        ns, c2, c3 = (cnt[1] + 1) // 2, cnt[2], cnt[3]
        return {
            "need": (ns, c2, c3, c3),
            "s_into_m": (ns // 2, c2 + (ns - ns // 2), c3, c3),
            "m_into_ll": (ns, c2 // 2, c3 + (c2 - c2 // 2), c3),
            "ll_into_lh": (ns, c2, c3 // 2, c3),
            "s_m_into_next": (ns // 2, c2 + (ns - ns // 2) - c2 // 2, c3 + c2 // 2, c3),
            "long": (ns + 7, c2 + 5, c3 + 3, c3),
        }
    if codec == "C2":
        cb = cnt[1]
        nn = cnt[0] + cnt[1]
        return {"need": (nn, cb), "a_into_h": (nn - cb // 2, cb), "long": (nn + 5, cb)}
    if codec == "C3":
        cs, cb = cnt[0], cnt[1]
        return {"need": (cs, cb, cb), "a_into_b": (cs // 2, cb + (cs - cs // 2), cb), "b_into_h": (cs, cb // 2, cb),
                "long": (cs + 5, cb + 3, cb)}
    if codec in ("C1", "VBZ"):
        return {"need": (cnt[0] + 2 * cnt[1],)}
    nib = cnt[1] + 2 * cnt[2] + 4 * cnt[3]  # VBZ0
    return {"need": ((nib + 1) // 2,)}


def _borrow(out):
    for codec in CODECS:
        k = len(_CLASSES[class_kind(codec)])
        for n in SMALL_SIZES + BIG_SIZES:
            for mix in (("uniform", "light") if n in SMALL_SIZES else ("uniform",)):
                rng = _rng("D", codec, n, mix)
                cls = draw_classes(rng, codec, n, mix)
                cnt = np.bincount(cls, minlength=k).tolist()
                keys = pack_keys(codec, cls)
                for tag, sizes in _borrow_sizes(codec, cnt).items():
                    if n in BIG_SIZES and tag not in ("s_m_into_next", "a_into_h", "a_into_b", "need"):
                        continue
                    if n in BIG_SIZES and tag == "need" and codec not in ("C1", "VBZ", "VBZ0"):
                        continue
                    parts = [keys] + [_rb(rng, s) for s in sizes]
                    out.append(Case(f"D_{codec}_{n}_{mix}_{tag}", "borrow", codec, n, frames_of(codec, parts), 0))
                if codec == "C1" and n > 8:  # the keys frame one byte short, the data frame one longer
                    parts = [keys] + [_rb(rng, cnt[0] + 2 * cnt[1])]
                    buf = b"".join(parts)
                    out.append(Case(f"D_{codec}_{n}_{mix}_keys_into_data", "borrow", codec, n,
                                    [buf[:len(keys) - 1], buf[len(keys) - 1:]], 0))


def _remaining(out):
    for codec in CODECS:
        for n in CORE_SIZES:
            for mix in ("uniform", "light"):
                rng = _rng("E", codec, n, mix)
                x = signal_of(draw_values(rng, codec, n, mix, last_big=True))
                parts = parts_of(codec, x)
                for extra in (1, 16):
                    p = parts[:-1] + [parts[-1] + _rb(rng, extra)]
                    out.append(Case(f"E_{codec}_{n}_{mix}_long{extra}", "remaining", codec, n, frames_of(codec, p), 4))
                if codec == "C5":
                    for m in (n - 1, n - 4):
                        out.append(Case(f"E_{codec}_{n}_{mix}_n{m - n}", "remaining", codec, m, frames_of(codec, parts),
                                        4))
                if mix == "uniform":
                    out.append(Case(f"E_{codec}_{n}_zero_samples", "remaining", codec, 0, frames_of(codec, parts), 4))
            if codec == "C1":  # one byte too many with no frame above n bytes: the chunk stays in the staged passes
                rng = _rng("E1", n)
                parts = parts_of(codec, signal_of(draw_values(rng, codec, n, "only0")))
                buf, kl = b"".join(parts) + _rb(rng, 1), len(parts[0])
                out.append(Case(f"E_{codec}_{n}_only0_long1_recut", "remaining", codec, n,
                                [buf[:kl + 1], buf[kl + 1:]], 4))


def _corrupt(out):
    for codec in APPLIES["corrupt"]:
        for n in CORE_SIZES:
            for mix in ("uniform", "light"):
                rng = _rng("F", codec, n, mix)
                x = signal_of(draw_values(rng, codec, n, mix, last_big=True))
                parts = parts_of(codec, x)
                p = parts[:-1] + [parts[-1][:-1]]
                out.append(Case(f"F_{codec}_{n}_{mix}_short1", "corrupt", codec, n, frames_of(codec, p), 6))
                # four samples more: for 1-bit keys only where that lengthens the keys (or, C1, needs data)
                if codec in TWO_BIT or codec == "C1" or key_len(codec, n + 4) > key_len(codec, n):
                    out.append(Case(f"F_{codec}_{n}_{mix}_nplus4", "corrupt", codec, n + 4, frames_of(codec, parts), 6))
            rng = _rng("F2", codec, n)
            if codec in FIVE:
                ns = (n + 1) // 2
                parts = [pack_keys(codec, [1] * n), _rb(rng, ns // 2), b"", b"", b""]
                out.append(Case(f"F_{codec}_{n}_all1_half_S", "corrupt", codec, n, parts, 6))
                parts = [pack_keys(codec, [3] * n), b"", b"", _rb(rng, n), b""]
                out.append(Case(f"F_{codec}_{n}_all3_no_Lhigh", "corrupt", codec, n, parts, 6))
            elif codec == "C2":
                out.append(Case(f"F_{codec}_{n}_allbig_no_H", "corrupt", codec, n,
                                [pack_keys(codec, [1] * n), _rb(rng, n), b""], 6))
            elif codec == "C3":
                out.append(Case(f"F_{codec}_{n}_allbig_no_H", "corrupt", codec, n,
                                [pack_keys(codec, [1] * n), b"", _rb(rng, n), b""], 6))


def _empty(out):
    for codec in CODECS:
        nf = 1 if codec in ONE_FRAME else O.VARIANT_FRAMES[codec]
        out.append(Case(f"G_{codec}_empty", "empty", codec, 0, [b""] * nf, 0))


def _vbz_pad(out):
    for n in CORE_SIZES:
        for mix in ("uniform", "only0"):
            rng = _rng("H", n, mix)
            x = signal_of(draw_values(rng, "VBZ", n, mix, last_big=True))
            buf = O.oracle_vbz_svb_encode(x)
            nk = key_len("VBZ", n)

            def add(tag, content, designed):
                out.append(Case(f"H_VBZ_{n}_{mix}_{tag}", "vbz_pad", "VBZ", n, [content], designed))

            if nk >= 17:
                add("keys_m17", buf[:nk - 17], 6)
            if nk >= 16:
                add("keys_m16", buf[:nk - 16], 4)
            add("keys_m1", buf[:nk - 1], 4)
            if len(buf) - nk >= 17:
                add("data_m1", buf[:-1], 4)  # the last value is two-byte: its high byte is missing
                add("data_m16", buf[:-16], 4)
                add("data_m17", buf[:-17], 6)
            else:
                add("data_m1", buf[:-1], 4)
            add("data_p1", buf + _rb(rng, 1), 4)
            add("data_p16", buf + _rb(rng, 16), 4)
        # a last value of one byte: nothing but that byte missing
        x = signal_of(draw_values(_rng("H1", n), "VBZ", n, "only0"))
        out.append(Case(f"H_VBZ_{n}_small_last_m1", "vbz_pad", "VBZ", n, [O.oracle_vbz_svb_encode(x)[:-1]], 4))
        # VBZ0: one frame, no padding
        rng = _rng("H0", n)
        x = signal_of(draw_values(rng, "VBZ0", n, "uniform", last_big=True))
        (buf,) = O.variant_streams("VBZ0", x)
        kl = key_len("VBZ0", n)
        out.append(Case(f"H_VBZ0_{n}_m1", "vbz_pad", "VBZ0", n, [buf[:-1]], 6))
        out.append(Case(f"H_VBZ0_{n}_p1", "vbz_pad", "VBZ0", n, [buf + _rb(rng, 1)], 4))
        out.append(Case(f"H_VBZ0_{n}_keys_m1", "vbz_pad", "VBZ0", n, [buf[:kl - 1]], 6))


_CAT = None


def catalogue():
    """Every case, built once per process (fixed seeds: the same cases in every process)."""
    global _CAT
    if _CAT is None:
        out = []
        for build in (_exact, _tail, _recut, _borrow, _remaining, _corrupt, _empty, _vbz_pad):
            build(out)
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        _CAT = out
    return _CAT


def cases(codec=None, family=None, max_n=None):
    return [c for c in catalogue() if (codec is None or c.codec == codec) and (family is None or c.family == family)
            and (max_n is None or c.n <= max_n)]
