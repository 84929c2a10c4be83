"""The catalogue of tests/_svb_cases.py checks itself (CPU): every case reaches the status it was built
for under the oracle; where the reference tree is present the reference's own compiled decoders read
the same samples and consume the same count from every case they can run on; and a plain per-sample
restatement of the seven walks, given one named fault at a time, shows that the catalogue tells each
fault from the true rule for every codec the fault applies to.

One thing the issue asked for cannot hold: by the documented claims rule (a frame's content above n
bytes) every VBZ blob that decodes n >= 1 samples is a claims chunk -- its one frame holds
svb16_key_length(n) + n bytes at least.  So VBZ has no family B or D case with claims == False; it has
the statuses 0 (the empty chunk), 4 and 6 there (family H), and tests/test_gpu_svb_cases.py reaches the
staged VBZ merge on families B and D through the bounded batch call, which has no claims pass.
"""
import collections

import numpy as np
import pytest

import _oracle as O
import _svb_cases as S
from test_oracle_ref import needs_ref

CAT = S.catalogue


def test_designed_status_and_samples():
    wrong = [f"{c.name}: oracle {c.rc}, designed {c.designed}" for c in CAT() if c.rc != c.designed]
    assert not wrong, wrong[:20]
    for c in CAT():
        if c.family in ("exact", "tail", "recut"):
            assert c.signal is not None and c.rc == 0 and np.array_equal(c.want, c.signal), c.name
        if c.family == "borrow":
            assert c.rc == 0, c.name


def test_every_family_for_every_codec_at_the_core_sizes():
    have = collections.Counter()
    for c in CAT():
        size = int(c.name.split("_")[2]) if c.name.split("_")[2].isdigit() else None
        have[(c.family, c.codec, size)] += 1
    for fam, codecs in S.APPLIES.items():
        for codec in codecs:
            if fam == "empty":
                assert have[(fam, codec, None)], (fam, codec)
                continue
            for n in S.CORE_SIZES:
                assert have[(fam, codec, n)], (fam, codec, n)
    for fam in ("exact", "borrow"):  # at every size
        for codec in S.CODECS:
            for n in S.SMALL_SIZES + S.BIG_SIZES:
                assert have[(fam, codec, n)], (fam, codec, n)


def test_staged_merges_are_reached():
    """Among the chunks that stay in the staged passes (claims == False): every status and, VBZ aside
    (module docstring), families B and D."""
    for codec in S.CODECS:
        stay = [c for c in CAT() if c.codec == codec and not c.claims]
        assert {0, 4, 6} <= {c.rc for c in stay}, (codec, collections.Counter(c.rc for c in stay))
        if codec != "VBZ":
            assert {"tail", "borrow"} <= {c.family for c in stay}, codec
    vbz = [c for c in CAT() if c.codec == "VBZ" and c.rc == 0 and c.n > 0]
    assert vbz and all(c.claims for c in vbz)
    # the claims pass is reached too, for the codec whose claims route is tested on its own
    assert sum(c.claims for c in CAT() if c.codec == "C5") >= 10


@needs_ref
def test_reference_decoders_agree_on_every_case_they_can_read():
    """Statuses 0 and 4: every read stays inside the buffer, so the reference's own decode_* runs on the
    case's buffer (followed by random padding, as test_oracle_ref._check_merge pads it) and must give the
    oracle's samples and consumed count."""
    rng = np.random.default_rng(5)
    seen = collections.Counter()
    for c in CAT():
        if c.designed not in (0, 4):
            continue
        inter, d, n = c.inter, c.d, c.n
        if c.codec == "VBZ":
            kl = S.key_len("VBZ", n)
            if kl > len(inter):
                # keys that end inside the padding: the reference's data reads then leave its buffer
                # (undefined; its SSE decoder asserts), and status 4 is the oracle's own rule for them
                continue
            got, cons = O.ref_vbz_svb_decode(inter, n)
            # the same walk as C1's over the content and its zero padding
            rc, want, cons_o = O.oracle_variant_merge("C1", inter + bytes(48), [kl, 0], n)
            if n == 0:
                cons_o = 0  # svb16/decode_scalar.hpp:43-45
            assert (cons == len(inter)) == (c.rc == 0), c.name
        else:
            if c.codec == "VBZ0":
                d = [len(inter)]
            pad = rng.integers(0, 256, 2 * n + 64, dtype=np.uint8).tobytes()
            got, cons = O.ref_variant_merge(c.codec, inter + pad, d, n)
            rc, want, cons_o = O.oracle_variant_merge(c.codec, inter + pad, d, n)
            assert (cons_o == len(inter)) == (c.rc == 0), c.name
        assert rc == O.OK, c.name
        assert np.array_equal(got, want), c.name
        assert cons == cons_o, (c.name, cons, cons_o)
        if c.rc == 0:
            assert np.array_equal(got, c.want), c.name
        seen[c.codec] += 1
    assert all(seen[k] > 20 for k in S.CODECS), seen


# ---- a per-sample restatement of the seven walks, with one optional fault -----------------------------
FAULTS = {
    "no_tail_mask": S.CODECS,
    "own_starts": ["C5", "C4", "C2", "C3"],
    "keys_from_frame": ["C5", "C4", "C1", "C2", "C3"],
    "remaining_first": S.CODECS,
    "content_bound": ["VBZ"],
}


class _Out(Exception):
    pass


def walk(codec, inter, d, n, fault=None):
    """(status, samples or None) of the merge of `inter` (the decoded frames back to back, sizes d)."""
    cs = len(inter)
    buf, limit = inter, cs
    two = codec in S.TWO_BIT
    per, bits = (4, 2) if two else (8, 1)
    kl = S.key_len(codec, n)
    oob = O.REMAINING if fault == "remaining_first" else O.CORRUPT
    if codec == "VBZ":
        buf = inter + bytes(S.VBZ_PADDING)
        limit = cs if fault == "content_bound" else cs + S.VBZ_PADDING
        if kl > cs:
            return (O.REMAINING if kl <= limit else oob), None
    # stream starts and bounds
    if codec in S.ONE_FRAME:
        mids = []
        first = kl
    else:
        mids = list(d[1:-1])
        first = d[0] if fault in ("keys_from_frame", "own_starts") else kl
    starts = [first]
    for m in mids:
        starts.append(starts[-1] + m)
    if fault == "own_starts":
        ends = [s + z for s, z in zip(starts, list(d[1:]))]
    else:
        ends = [limit] * len(starts)
    pos = list(starts)

    def rd(s):
        if pos[s] >= ends[s] or pos[s] >= limit:
            raise _Out
        v = buf[pos[s]]
        pos[s] += 1
        return v

    nib = [0]

    def rd_nib(s):  # nibbles of stream s, low first
        p = starts[s] + (nib[0] >> 1)
        if p >= ends[s] or p >= limit:
            raise _Out
        v = (buf[p] >> 4) if nib[0] & 1 else (buf[p] & 15)
        nib[0] += 1
        return v

    ncodes = kl * per if fault == "no_tail_mask" else n
    out = np.zeros(n, np.int16)
    prev = 0
    o1, o2, o3 = (0, 0, 0) if codec == "C4" else (1, 17, 273)
    try:
        for i in range(ncodes):
            kb = i // per
            if kb >= limit:
                raise _Out
            c = (buf[kb] >> (bits * (i % per))) & (3 if two else 1)
            if codec in S.FIVE:
                if c == 0:
                    v = 0
                elif c == 1:
                    v = rd_nib(0) + o1
                elif c == 2:
                    v = rd(1) + o2
                else:
                    lo = rd(2)
                    v = (rd(3) << 8) + lo + o3
            elif codec == "VBZ0":
                v = 0
                for k in range((0, 1, 2, 4)[c]):
                    v |= rd_nib(0) << (4 * k)
                v = 0 if c == 0 else v + (0, 1, 17, 273)[c]
            elif codec == "C2":
                v = rd(0)
                if c:
                    v |= rd(1) << 8
            elif codec == "C3":
                if c:
                    lo = rd(1)
                    v = lo | (rd(2) << 8)
                else:
                    v = rd(0)
            else:  # C1, VBZ
                if c:
                    if pos[0] + 1 >= limit:
                        raise _Out
                    lo = rd(0)
                    v = lo | (rd(0) << 8)
                else:
                    v = rd(0)
            v &= 0xFFFF
            prev = (prev + ((v >> 1) ^ -(v & 1))) & 0xFFFF
            if i < n:
                out[i] = np.uint16(prev).astype(np.int16)
    except _Out:
        return oob, None
    if codec in S.FIVE:
        consumed = pos[3]
    elif codec == "C2":
        consumed = pos[1] if n else kl
    elif codec == "C3":
        consumed = pos[2] if n else kl
    elif codec == "VBZ0":
        consumed = starts[0] + (nib[0] + 1) // 2 if n else 0
    else:
        consumed = pos[0] if n or codec == "C1" else 0
    return (O.OK if consumed == cs else O.REMAINING), out


SMALL = 5000


def test_restatement_agrees_with_the_oracle():
    k = 0
    for c in S.cases(max_n=SMALL):
        st, out = walk(c.codec, c.inter, c.d, c.n)
        assert st == c.rc, (c.name, st, c.rc)
        if c.rc == 0:
            assert np.array_equal(out, c.want), c.name
        k += 1
    assert k > 1000


@pytest.mark.parametrize("fault", list(FAULTS))
def test_every_fault_is_caught_for_every_codec(fault):
    """A merge with this fault differs from the oracle on some case of every codec it applies to: in its
    status, or in its samples where the status is 0."""
    for codec in FAULTS[fault]:
        caught = None
        # the small cases first: one catch is enough
        for c in sorted(S.cases(codec=codec, max_n=SMALL), key=lambda c: c.n):
            st, out = walk(c.codec, c.inter, c.d, c.n, fault)
            if st != c.rc or (c.rc == 0 and not np.array_equal(out, c.want)):
                caught = c.name
                break
        assert caught, (fault, codec)
