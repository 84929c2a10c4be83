"""How often the table description's own bounds decide "raw" before its FSE chains run, per C5 stream,
over N bench-generator reads (seed 42, 100,000 samples): tools/desc_bound_probe.hip has the build line."""
import collections
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import _oracle as O

P = C.CDLL(os.path.join(ROOT, "_ab", "libdesc_bound_probe.so"))
P.probe.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
stats = collections.Counter()
margin = []
for r in range(N):
    x = O.synth_read(r, 100_000)
    st = O.c5_streams(x)
    for si, name in enumerate(["keys", "S", "M", "Llow", "Lhigh"]):
        a = np.frombuffer(st[si], np.uint8).copy()
        out = np.zeros(16, np.int64)
        full = P.probe(a.ctypes.data, a.size, out.ctypes.data)
        if not full:
            stats[(name, "no-table")] += 1
            continue
        _, n, maxSym, largest, cs, minGain, hSize, hLow, hHigh, nh, tl, raw, wt = [int(v) for v in out[:13]]
        T = n - minGain - cs
        # the early decision
        fire = False
        if hLow >= 0:
            if hLow >= maxSym // 2 and maxSym > 128:
                fire = True
            elif hLow + 1 >= T and (maxSym > 128 or (maxSym + 1) // 2 + 1 >= T):
                fire = True
        if fire:
            assert raw, (name, r, out)
        stats[(name, "raw" if raw else "huf", "fire" if fire else "nofire")] += 1
        if name == "Llow":
            margin.append((hLow + 1 - T, hSize - T, hHigh + 1 - T, hLow, hSize, hHigh))
for k in sorted(stats):
    print(k, stats[k])
m = np.array(margin)
print("Llow: hLow+1-T min/med/max", m[:, 0].min(), np.median(m[:, 0]), m[:, 0].max())
print("Llow: hSize-T  min/med/max", m[:, 1].min(), np.median(m[:, 1]), m[:, 1].max())
print("Llow: hLow,hSize-1,hHigh sample", m[:5, 3:])
print("bracket ok:", bool(((m[:, 3] <= m[:, 4] - 1) & (m[:, 4] - 1 <= m[:, 5])).all()))
