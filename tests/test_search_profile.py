"""What the match-search cases (_search_cases.py) are and what they reach, on the host: every stream is
the M stream of its chunk, the oracle accepts the chunk and its M frame is ZSTD_compress(stream, 1),
the host model writes the same frame, and the search profile (z1m_search_profile, a restatement of the
serial search with the wave search's bookkeeping) yields the model's sequences.  The floors below are
conditions on the inputs: they say how often the case set takes each path of fast_search_wave
(csrc/pgn_zenc.h) that a wrong bound would break without any round trip noticing.  No GPU here;
tests/test_gpu_search.py runs the same set on one."""
import functools

import numpy as np

import _oracle as O
import _search_cases as S
from _search_cases import BACK, K, KIND, LL, MLEN, NFALSE, OFFSET, MLBASE, POS, POST_REP, REP_IP2, SAME_ROUND, TABLE, TO_END
from test_gpu_enc_tables import m_signal, model_sequences


@functools.lru_cache(maxsize=None)
def profiles():
    """name -> rows, or None for a stream the certificate covers (the GPU search does not run)."""
    return {n: (None if S.certified(s) else S.profile(s)) for n, s in S.profiled_cases().items()}


def searched():
    return {n: r for n, r in profiles().items() if r is not None}


def all_rows(names=None):
    rows = [r for n, r in searched().items() if len(r) and (names is None or n in names)]
    return np.concatenate(rows)


def first_hits(rows):
    """Rows found by a round's ballot (not the post-match repcode loop)."""
    return rows[rows[:, KIND] != POST_REP]


def test_set_size():
    c = S.cases()
    assert len(c) == len(S.profiled_cases()) + len(S.large_cases())
    assert 120 <= len(c) <= 220
    assert sum(len(s) for s in c.values()) < 8_000_000
    assert all(len(s) <= 131072 for s in S.profiled_cases().values())
    assert all(len(s) > 131072 for s in S.large_cases().values())


def test_streams_are_the_chunks_m_streams():
    for name, s in S.cases().items():
        assert O.c5_streams(m_signal(s))[2] == s, name


def test_oracle_accepts_and_m_frame_is_zstd():
    for name, (x, blob, st) in S.reference().items():  # reference() asserts status 0
        fr = O.zstd_compress1(S.cases()[name])
        assert int(st[7]) == len(fr), name
        assert S.m_frame_of(blob, st) == fr, name


def test_model_writes_the_same_frame():
    for name, s in S.cases().items():
        assert S.model_compress(s) == O.zstd_compress1(s), name


def test_profile_restates_the_model_search():
    """Pinned on every profiled case, certified or not: the rows' (litLength, offset, matchLength - 3) are
    z1m_sequences', and the rows are consistent with themselves."""
    for name, s in S.profiled_cases().items():
        r = S.profile(s)
        sq = model_sequences(s)
        assert len(r) == len(sq), name
        assert not (len(r) and S.certified(s)), f"{name}: certified, yet the search finds sequences"
        if not len(r):
            continue
        assert np.array_equal(r[:, [LL, OFFSET, MLBASE]], sq.astype(np.int64)), name
        assert (r[:, MLEN] == r[:, MLBASE] + 3).all(), name
        assert ((r[:, POS] + r[:, MLEN] == len(s)) == (r[:, TO_END] == 1)).all(), name
        pos = np.concatenate([[0], (r[:, POS] + r[:, MLEN])[:-1]]) + r[:, LL]  # anchor + literals
        assert np.array_equal(pos, r[:, POS]), name


def test_sequences_reach_the_frame():
    """A block that gains too little is written raw and hides what the search found: every case with
    sequences, the uniform ones apart, is a compressed block in the oracle's frame."""
    for name, r in searched().items():
        if len(r) and not name.startswith("uniform/"):
            assert S.compressed_block(S.profiled_cases()[name]), name


def test_certified_and_uncertified_noise():
    prof = profiles()
    uni = [n for n in prof if n.startswith("uniform/")]
    assert sum(prof[n] is None for n in uni) >= 1
    assert sum(prof[n] is not None for n in uni) >= 10
    # what the uniform streams are for: the certificate, or the exact search with (next to) nothing found
    assert all(prof[n] is None or len(prof[n]) <= 2 for n in uni)


def test_same_round_candidates():
    rows = all_rows()
    assert (rows[:, KIND] == SAME_ROUND).sum() >= 100


def test_false_fingerprints():
    rows = first_hits(all_rows())
    assert rows[:, NFALSE].sum() >= 200
    wide = [n for n in searched() if len(S.profiled_cases()[n]) in S.WIDE_SIZES]
    assert first_hits(all_rows(set(wide)))[:, NFALSE].sum() >= 20  # the 7-bit fingerprint
    # a real hit later in the round of a dropped false candidate
    assert ((rows[:, NFALSE] > 0) & (rows[:, KIND] != REP_IP2)).sum() >= 100


def test_false_candidate_with_three_equal_bytes():
    """The acceptance threshold of the drop-and-retry loop (nm >= 4): a same-slot, same-fingerprint table
    candidate whose first 3 bytes are the position's and whose 4th is not, dropped in the round of a real
    match.  Accepted at 3 bytes it would be a sequence of its own, so the frame would differ."""
    s = S.profiled_cases()["false3/pair"]
    a = np.frombuffer(s, np.uint8)
    A, B = a[S.FALSE_A:S.FALSE_A + 6], a[S.FALSE_B:S.FALSE_B + 6]
    assert (A[:3] == B[:3]).all() and A[3] != B[3]
    assert S.hash6_13(S._le(A[None, :]))[0] == S.hash6_13(S._le(B[None, :]))[0]
    assert S.entry_fp(S._le(A[None, :]), len(s))[0] == S.entry_fp(S._le(B[None, :]), len(s))[0]
    rows = S.false_prefix_rows(s, 3)
    assert len(rows) == 1 and rows[0][NFALSE] == 1 and rows[0][KIND] == TABLE
    r = searched()["false3/pair"]
    assert not ((r[:, POS] <= S.FALSE_B) & (r[:, POS] + r[:, MLEN] > S.FALSE_B)).any()  # no real match covers it


def test_fingerprint_layouts_share_the_false_candidates():
    """Both entry layouts meet false candidates: the issue sets >= 20 for the 7-bit fingerprint
    (test_false_fingerprints); the same floor holds for the 10-bit one, which most frames use."""
    narrow = {n for n in searched() if len(S.profiled_cases()[n]) + 2 < (1 << 17)}
    assert first_hits(all_rows(narrow))[:, NFALSE].sum() >= 20


def test_backward_extensions():
    rows = all_rows()
    assert (rows[:, BACK] >= 64).sum() >= 20
    assert (rows[:, BACK] >= 128).sum() >= 20
    for b in S.BACKS:
        r = searched()[f"back/{b}"]
        assert (r[:, BACK] == b).sum() == 1, b
    assert S.anchor_stopped_rows(S.profiled_cases()["back/anchor_stop"])


def test_matches_at_and_near_the_end():
    """Every directed length ends at the stream's end (from 8 bytes: _search_cases.END_LENGTHS_AT_END says
    why no shorter match can) and 1 .. 9 bytes before it."""
    n = S.N_DIRECTED
    gaps = set()
    for length in S.END_LENGTHS:
        if length in S.END_LENGTHS_AT_END:
            last = searched()[f"end/{length}_at_end"][-1]
            assert last[MLEN] == length and last[TO_END] == 1 and last[POS] == n - length, length
        g = S.gap_before_end(length)
        gaps.add(g)
        last = searched()[f"end/{length}_gap{g}"][-1]
        assert last[MLEN] == length and last[TO_END] == 0 and last[POS] + length == n - g, length
    assert S.END_LENGTHS_AT_END == tuple(l for l in S.END_LENGTHS if l >= 8)
    assert gaps == set(range(1, 10))


def test_first_hits_by_lane():
    rows = first_hits(all_rows())
    lane = rows[:, K] % 64
    assert (lane == 63).sum() >= 3
    assert (lane == 62).sum() >= 3
    assert ((lane == 0) & (rows[:, K] >= 64)).sum() >= 3
    for l in S.LANES:  # the directed streams alone, and both kinds of candidate in the last lanes
        r = first_hits(searched()[f"lane/{l}"])
        mine = r[(r[:, K] % 64 == l) & ((r[:, K] >= 64) | (l > 0))]
        assert len(mine) >= 3, l
        assert (mine[:, KIND] == TABLE).any(), l
        if l:
            assert (mine[:, KIND] == SAME_ROUND).any(), l


def test_repcodes():
    rows = all_rows()
    assert (rows[:, KIND] == REP_IP2).sum() >= 100
    assert (rows[:, KIND] == POST_REP).sum() >= 100
    assert ((rows[:, KIND] == POST_REP) & (rows[:, LL] == 0)).sum() == (rows[:, KIND] == POST_REP).sum()


def test_generators_at_every_size():
    names = set(S.profiled_cases())
    for g, sizes in S.GRID.items():
        for n in sizes:
            assert f"{g}/{n}" in names
    for n in S.SINGLE_SIZES + S.WIDE_SIZES:
        assert any(f"{g}/{n}" in names for g in S.GRID), n
    big = set(S.large_cases())
    for g in ("word_soup", "late_copy"):
        for n in S.MULTI_SIZES:
            assert f"{g}/{n}" in big
    assert {f"word_soup/{n}" for n in S.PAIR_SIZES} <= big
