#!/usr/bin/env python3
"""Typed record tags (tags.*, pgn_bam_records_tagged_device) against the old record call and against splicing the
tags in on the host, on bam_timing's batch: 100,000 reads of 6,400 bases and 16,000 frames, with the move table.
One process, HIP events on the codec's stream.

Quantities (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps; the two calls of a
pair alternate run by run, the old call first):
  1  the typed path itself: the tagged call with two U32 columns against the old call with the same two, raw and
     BGZF.  The old call is the parent's code, so it is the yardstick.  Condition: the difference of the means stays
     inside the two calls' combined run-to-run spread ((max - min) of the one plus (max - min) of the other).
  2  a full set of ten columns: qs:f ch:I rn:I ts:i ns:i sm:f sd:f du:f, BC:Z from a 97-entry dictionary of 60-byte
     names, pi:Z as a 36-byte string per read; time and ps per output byte, raw and BGZF.
  3  whether the feature pays.  Device route: the tagged raw records of 2.  Host route, what a user does today: the
     old call with the unsigned columns (ch, rn), the download, then the other eight tags spliced into every record
     in front of mv with block_size fixed up, in 16 threads.  Condition: the device route wins by more than the two
     routes' combined spread.  The download that both routes need before a file is written is also given alone.
Before any time counts, the identity of 1 is checked in full (bytes, rec_off, status, written), sampled reads' records
of 2 against bam_records_tagged_signal, and the host route's spliced bytes against the device route's in full.  The
tool prints the verdicts and changes nothing to make them hold.

    python tools/tagged_records_timing.py [--reads N] [--bases M] [--frames F] [--runs R] [--steps K] [--out FILE]
"""
import argparse
import os
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch

    import bench
    from rawnanoporesignalcompression_amd import DecodedReads, PGNanoCodec, bam, tags

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--bases", type=int, default=6_400)
    p.add_argument("--frames", type=int, default=16_000)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def one_run(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sum(ms) / len(ms)

    def paired(first, second):
        a, b = [], []
        for _ in range(args.runs):
            a.append(one_run(first))
            b.append(one_run(second))
        return a, b

    mean = lambda runs: sum(runs) / len(runs)
    spread = lambda runs: max(runs) - min(runs)
    fmt = lambda name, runs: f"{name} {mean(runs):9.3f} ms (runs " + ", ".join(f"{v:.3f}" for v in runs) + ")"
    N, M, F = args.reads, args.bases, args.frames
    total, nframes = N * M, N * F
    say(f"tagged_records_timing: {torch.cuda.get_device_name(0)}, {N} reads of {M} bases and {F} frames, with moves, "
        f"{args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    say(f"stream_copy_gbs {bench.stream_copy_gbs(torch):.1f} (read + write bytes of a device-to-device copy)")
    codec = PGNanoCodec(0)
    rng = np.random.default_rng(args.seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (total,), device=dev, generator=gen)]
    qual = torch.randint(33, 84, (total,), device=dev, generator=gen, dtype=torch.uint8)
    codes = torch.randint(0, 4, (nframes,), device=dev, generator=gen, dtype=torch.uint8)
    codes |= (torch.rand(nframes, device=dev, generator=gen) < 0.4).to(torch.uint8) << 7
    ids_host = rng.integers(0, 256, (N, 16)).astype(np.uint8)
    ids = torch.from_numpy(ids_host).to(dev)
    rb = torch.arange(N + 1, device=dev, dtype=torch.int64) * M
    rf = torch.arange(N + 1, device=dev, dtype=torch.int64) * F
    decoded = DecodedReads(seq, rb, torch.zeros(N, dtype=torch.int32, device=dev), None, None, None, None)
    mv = (codes, rf, 5)
    up = lambda a: torch.from_numpy(a).to(dev)
    host = {"qs": rng.uniform(5, 30, N).astype(np.float32), "ch": rng.integers(1, 3001, N).astype(np.int32),
            "rn": rng.integers(0, 200_000, N).astype(np.int32), "ts": rng.integers(-50, 4000, N).astype(np.int32),
            "ns": rng.integers(20_000, 200_000, N).astype(np.int32), "sm": rng.normal(90, 5, N).astype(np.float32),
            "sd": rng.normal(15, 2, N).astype(np.float32), "du": rng.uniform(1, 60, N).astype(np.float32)}
    names = [(b"4e7d2c8a1f3b_2026-01-01_kit-barcode%02d_" % k).ljust(60, b"x") for k in range(97)]
    bc_host = rng.integers(0, 97, N).astype(np.int32)
    pi_host = np.frombuffer(b"".join(b"%08x-%04x-%04x-%04x-%012x" % tuple(int(v) for v in row) for row in
                                     zip(rng.integers(0, 2**32, N), rng.integers(0, 2**16, N), rng.integers(0, 2**16, N),
                                         rng.integers(0, 2**16, N), rng.integers(0, 2**48, N))), np.uint8)
    assert len(pi_host) == 36 * N
    d = {k: up(v) for k, v in host.items()}
    two_plain = {"qs": d["rn"], "ch": d["ch"]}
    two_typed = {k: tags.u32(v) for k, v in two_plain.items()}
    table = tags.StringTable(names).to(dev)
    full = {"qs": tags.f32(d["qs"]), "ch": d["ch"], "rn": d["rn"], "ts": tags.i32(d["ts"]), "ns": tags.i32(d["ns"]),
            "sm": tags.f32(d["sm"]), "sd": tags.f32(d["sd"]), "du": tags.f32(d["du"]), "BC": tags.zdict(up(bc_host), table),
            "pi": tags.zstr(up(np.arange(N + 1, dtype=np.int32) * 36), up(pi_host))}
    unsigned = {"ch": d["ch"], "rn": d["rn"]}
    bound = bam.bam_bound_tagged(N, total, list(full.values()), nframes)
    out = torch.empty(bam.bgzf_bound(bound), dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)
    call = lambda t, bgzf, o=out: bam.bam_records(codec, decoded, qual, ids, t, moves=mv, bgzf=bgzf, out=o, stream=codec.stream)

    # ---- 1: the typed path itself --------------------------------------------------------------------------------
    for bgzf, label in ((False, "raw"), (True, "BGZF")):
        old, new = call(two_plain, bgzf), call(two_typed, bgzf, out2)
        torch.cuda.synchronize()
        nb = int(old.written[1].item())
        same = all(torch.equal(getattr(old, f), getattr(new, f)) for f in ("rec_off", "status", "written"))
        same = same and bool(torch.equal(out[:nb], out2[:nb])) and bool((old.status == 0).all())
        say(f"1 {label}: two U32 columns, {nb} bytes; every output of the tagged call equals the old call's: {same}")
        a, b = paired(lambda: call(two_plain, bgzf), lambda: call(two_typed, bgzf))
        diff, both = mean(b) - mean(a), spread(a) + spread(b)
        say("  " + fmt("old call   ", a) + f", {mean(a) * 1e9 / nb:.3f} ps per output byte")
        say("  " + fmt("tagged call", b) + f", {mean(b) * 1e9 / nb:.3f} ps per output byte")
        say(f"  condition: |tagged - old| = {abs(diff):.3f} ms ({diff / mean(a) * 100:+.2f} %) within the combined spread "
            f"{both:.3f} ms: {abs(diff) <= both}")
    del out2

    # ---- 2: a full set --------------------------------------------------------------------------------------------
    results = {}
    for bgzf, label in ((False, "raw"), (True, "BGZF")):
        rec = call(full, bgzf)
        torch.cuda.synchronize()
        W, nb = (int(v) for v in rec.written.cpu().numpy())
        ok = bool((rec.status == 0).all())
        if not bgzf:
            off_host = rec.rec_off.cpu().numpy()
            for r in sorted(set([0, 1, N // 2, N - 1] + rng.integers(0, N, 8).tolist())):
                a, b = r * M, (r + 1) * M
                one = {k: v[r:r + 1] for k, v in host.items()}
                cols = {"qs": tags.f32(one["qs"]), "ch": one["ch"].view(np.uint32), "rn": one["rn"].view(np.uint32),
                        "ts": tags.i32(one["ts"]), "ns": tags.i32(one["ns"]), "sm": tags.f32(one["sm"]), "sd": tags.f32(one["sd"]),
                        "du": tags.f32(one["du"]), "BC": tags.zdict(bc_host[r:r + 1], names),
                        "pi": tags.zstr([pi_host[36 * r:36 * r + 36].tobytes()])}
                want = tags.bam_records_tagged_signal(
                    ids_host[r:r + 1], seq[a:b].cpu().numpy(), qual[a:b].cpu().numpy(), [0, M], [0], cols,
                    moves=(codes[r * F:(r + 1) * F].cpu().numpy(), [0, F], 5))[0]
                ok = ok and out[int(off_host[r]):int(off_host[r + 1])].cpu().numpy().tobytes() == want
        t = [one_run(lambda: call(full, bgzf)) for _ in range(args.runs)]
        results[label] = (t, W, nb)
        say("2 " + fmt(f"tagged call, ten columns, {label}", t) + f": {nb} bytes, {mean(t) * 1e9 / nb:.3f} ps per output byte"
            + (f"; statuses 0 and sampled records equal the host model's: {ok}" if not bgzf else f"; statuses all 0: {ok}"))

    # ---- 3: the device route against the host route ------------------------------------------------------------------
    t_dev, W_dev, _ = results["raw"]
    call(full, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_host = out[:W_dev].cpu().numpy()
    t_down_dev = (time.perf_counter() - t0) * 1e3
    want_off = call(full, False).rec_off.cpu().numpy()
    name_at = np.zeros(98, np.int64)
    name_at[1:] = np.cumsum([len(s) for s in names])
    blob = b"".join(names)
    pack = struct.Struct("<2sBf2sBi2sBi2sBf2sBf2sBf")

    def splice(raw, off, lo, hi, parts):
        view = memoryview(raw)
        for r in range(lo, hi):
            a, b = int(off[r]), int(off[r + 1])
            cut = b - (9 + F)                                   # mv stays last; ch and rn are in front of the cut
            front = 73 + (M + 1) // 2 + M
            extra = pack.pack(b"qs", 0x66, host["qs"][r], b"ts", 0x69, host["ts"][r], b"ns", 0x69, host["ns"][r],
                              b"sm", 0x66, host["sm"][r], b"sd", 0x66, host["sd"][r], b"du", 0x66, host["du"][r])
            k = int(bc_host[r])
            z = b"BCZ" + blob[name_at[k]:name_at[k + 1]] + b"\0piZ" + pi_host[36 * r:36 * r + 36].tobytes() + b"\0"
            size = (b - a - 4) + len(extra) + len(z)
            # the device's column order: qs ch rn ts ns sm sd du BC pi
            parts[r] = b"".join((struct.pack("<I", size), view[a + 4:a + front], extra[:7], view[a + front:cut], extra[7:], z,
                                 view[cut:b]))

    th, t_old, t_down = [], [], []
    spliced = None
    with ThreadPoolExecutor(args.threads) as pool:
        for _ in range(args.runs):
            t_old.append(one_run(lambda: call(unsigned, False)))
            rec = call(unsigned, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            W = int(rec.written[0].item())
            raw_host = out[:W].cpu().numpy()
            off_host = rec.rec_off.cpu().numpy()
            t_down.append((time.perf_counter() - t0) * 1e3)
            parts = [None] * N
            per = -(-N // args.threads)
            t0 = time.perf_counter()
            list(pool.map(lambda i: splice(raw_host, off_host, i * per, min((i + 1) * per, N), parts), range(args.threads)))
            spliced = b"".join(parts)
            th.append((time.perf_counter() - t0) * 1e3)
    same = np.array_equal(np.frombuffer(spliced, np.uint8), want_host)
    same = same and np.array_equal(np.cumsum([0] + [len(x) for x in parts]), want_off.view(np.int64))
    del parts, spliced
    host_route = [a + b + c for a, b, c in zip(t_old, t_down, th)]
    say("3 " + fmt("device route: tagged raw records", t_dev) + f" (then a download of {W_dev} bytes: {t_down_dev:.0f} ms)")
    say("  " + fmt("host route: old call with ch, rn   ", t_old))
    say("  " + fmt("            download                ", t_down))
    say("  " + fmt(f"            splice in {args.threads} threads    ", th) + f"; its bytes equal the device route's: {same}")
    say("  " + fmt("            in all                  ", host_route))
    both = spread(t_dev) + spread(host_route)
    say(f"  condition: the device route wins by more than the combined spread: {mean(host_route) - mean(t_dev) > both} "
        f"(host - device = {mean(host_route) - mean(t_dev):.3f} ms, combined spread {both:.3f} ms, host / device = "
        f"{mean(host_route) / mean(t_dev):.0f}; the splice alone / device = {mean(th) / mean(t_dev):.0f})")
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
