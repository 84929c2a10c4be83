"""Which paths of the GPU match search the GPU suite's inputs take, counted on the host with the search
profile (csrc/model_capi.hip z1m_search_profile): the rows of the table in DESIGN.md section 3.  Counts
are over single-block streams; a stream the no-match certificate covers never runs the search.  "False
fingerprints" are table candidates with the entry's fingerprint and other bytes, looked up at or before a
hit in its round of 64 visits.  No GPU needed:  python tools/search_profile_table.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import _oracle as O  # noqa: E402
import _search_cases as S  # noqa: E402
from _search_cases import BACK, K, KIND, NFALSE, POST_REP, REP_IP2, SAME_ROUND  # noqa: E402


def report(title, streams):
    searched = certified = 0
    t = dict.fromkeys(("same_round", "false_fp", "back64", "back128", "lane63", "lane62", "lane0", "rep_ip2", "post_rep"), 0)
    for s in streams:
        if len(s) < 7 or len(s) > 131072:
            continue
        if S.certified(s):
            certified += 1
            continue
        searched += 1
        r = S.profile(s)
        if not len(r):
            continue
        fh = r[r[:, KIND] != POST_REP]
        t["same_round"] += int((r[:, KIND] == SAME_ROUND).sum())
        t["false_fp"] += int(fh[:, NFALSE].sum())
        t["back64"] += int((r[:, BACK] >= 64).sum())
        t["back128"] += int((r[:, BACK] >= 128).sum())
        t["lane63"] += int((fh[:, K] % 64 == 63).sum())
        t["lane62"] += int((fh[:, K] % 64 == 62).sum())
        t["lane0"] += int(((fh[:, K] % 64 == 0) & (fh[:, K] >= 64)).sum())
        t["rep_ip2"] += int((r[:, KIND] == REP_IP2).sum())
        t["post_rep"] += int((r[:, KIND] == POST_REP).sum())
    print(f"{title}: exact-searched {searched} / certified {certified}  " + "  ".join(f"{k} {v}" for k, v in t.items()))


def main():
    import test_gpu_enc_tables as E
    import test_gpu_parity as P

    ss = []
    for r in range(40):
        ss += O.c5_streams(O.synth_read(r, 100000))
    report("40 synthetic reads x 100,000", ss)
    rng = np.random.default_rng(11)
    ss = []
    for r, n in enumerate(rng.integers(0, 40000, 300)):
        ss += O.c5_streams(O.synth_read(r, int(n)))
    report("test_batch_device_identical (300 reads)", ss)
    ss = []
    for x in P._pattern_signals().values():
        ss += O.c5_streams(x)
    report("_pattern_signals", ss)
    report("test_gpu_enc_tables.cases()", list(E.cases().values()))
    pc = S.profiled_cases()
    report("_search_cases.profiled_cases()", list(pc.values()))
    report("  of these, 20-bit index / 7-bit fingerprint", [s for s in pc.values() if len(s) + 2 >= 1 << 17])


if __name__ == "__main__":
    main()
