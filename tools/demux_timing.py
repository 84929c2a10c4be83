#!/usr/bin/env python3
"""Adapters and barcodes (demux.find_patterns, demux.classify, demux.trim_reads) against the record-and-deflate step
they feed, at the BAM timing's batch: 100,000 reads of 6,400 bases and 16,000 frames, 96 barcodes as head and tail
patterns of 40 to 90 bytes (192 patterns), four adapters, W = 150.  One process, HIP events on the codec's stream.

Every read carries a head adapter and, nine in ten, a barcode between its flanks with 0 to 3 substitutions, and the
barcode's reverse complement and a tail adapter at the far end, so that hits are as few as in a real run: one
barcode in 96 matches a given read.

Quantities (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  f    find_patterns: the per-side index with a side's patterns of at most 64 bytes first, and waves that hold such
       patterns alone running the column's first word only (the default)
  p    find_patterns, the other form (PGN_DEMUX_FIND=plain, a second context): the index in pattern order and both
       words in every wave; the two forms' outputs are compared in full
  c    classify
  t    trim_reads with qualities and the move table
  r    bam_records (raw, with the move table) + bgzf_deflate of the trimmed batch: the step the three calls feed
  h    the host route on a sample of reads: the download of all bases (timed once), then find_patterns_signal of
       `--host-reads` reads in `--threads` threads, scaled to the batch and labelled as scaled
Before any time counts, sampled reads' hits are compared with find_patterns_signal, and the classes and the cut reads
with the planted barcodes and inserts.  Condition: f + c + t < r, so that the route's longest step does not move.
The tool prints the verdict and changes nothing to make it hold.

    python tools/demux_timing.py [--reads N] [--bases M] [--frames F] [--runs R] [--steps K] [--out FILE]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch

    import bench
    from rawnanoporesignalcompression_amd import DecodedReads, PGNanoCodec, bam, bgzf, demux, host

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--bases", type=int, default=6_400)
    p.add_argument("--frames", type=int, default=16_000)
    p.add_argument("--barcodes", type=int, default=96)
    p.add_argument("--window", type=int, default=150)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--host-reads", type=int, default=64)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        runs = []
        for _ in range(args.runs):
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
            runs.append(sum(ms) / len(ms))
        return runs

    mean = lambda runs: sum(runs) / len(runs)
    fmt = lambda name, runs: f"{name} {mean(runs):9.3f} ms (runs " + ", ".join(f"{v:.3f}" for v in runs) + ")"
    N, M, F, NB, W = args.reads, args.bases, args.frames, args.barcodes, args.window
    total, nframes = N * M, N * F
    say(f"demux_timing: {torch.cuda.get_device_name(0)}, {N} reads of {M} bases and {F} frames, {NB} barcodes as head and "
        f"tail patterns, four adapters, W = {W}, {args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    say(f"stream_copy_gbs {bench.stream_copy_gbs(torch):.1f} (read + write bytes of a device-to-device copy)")
    codec = PGNanoCodec(0)
    os.environ["PGN_DEMUX_FIND"] = "plain"
    plain = PGNanoCodec(0)
    del os.environ["PGN_DEMUX_FIND"]
    rng = np.random.default_rng(args.seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    rand_seq = lambda n: letters[rng.integers(0, 4, n)].tobytes()
    front, rear = rand_seq(12), rand_seq(12)
    barcodes = [rand_seq(int(k)) for k in rng.integers(16, 67, NB)]         # with the flanks: 40 to 90 bytes
    head_adapters, tail_adapters = [rand_seq(28), rand_seq(22)], [rand_seq(28), rand_seq(22)]
    sets = (demux.barcode_patterns(front, barcodes, rear, max_dist=9) +
            demux.adapter_patterns(head=head_adapters, tail=tail_adapters, max_dist=5))
    lens = [len(q) for q in sets.patterns]
    say(f"patterns: {len(sets)} of {min(lens)} to {max(lens)} bytes, {sum(lens)} bytes in all")
    pats = sets.to(0)

    # the batch: random bases, then the planted ends written over them on the device from a host table of pastes
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (total,), device=dev, generator=gen)]
    qual = torch.randint(33, 84, (total,), device=dev, generator=gen, dtype=torch.uint8)
    planted = np.where(rng.random(N) < 0.9, rng.integers(0, NB, N), -1)
    head_len, tail_len = np.zeros(N, np.int64), np.zeros(N, np.int64)
    width = 160
    heads, tails = np.zeros((N, width), np.uint8), np.zeros((N, width), np.uint8)

    def noisy(s, k):
        s = bytearray(s)
        for at in rng.integers(3, len(s) - 3, k):
            s[at] = letters[(b"ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
        return bytes(s)

    fulls = [front + b + rear for b in barcodes]
    for r in range(N):
        c = int(planted[r])
        h = noisy(head_adapters[r & 1], int(rng.integers(0, 3)))
        t = noisy(tail_adapters[r & 1], int(rng.integers(0, 3)))
        if c >= 0:
            h += noisy(fulls[c], int(rng.integers(0, 4)))
            t = noisy(demux.revcomp(fulls[c]), int(rng.integers(0, 4))) + t
        head_len[r], tail_len[r] = len(h), len(t)
        heads[r, :len(h)] = np.frombuffer(h, np.uint8)
        tails[r, width - len(t):] = np.frombuffer(t, np.uint8)
    view = seq.view(N, M)
    d_heads, d_tails = torch.from_numpy(heads).to(dev), torch.from_numpy(tails).to(dev)
    view[:, :width] = torch.where(d_heads != 0, d_heads, view[:, :width])
    view[:, M - width:] = torch.where(d_tails != 0, d_tails, view[:, M - width:])
    del d_heads, d_tails

    # frames: F per read, a base every F / M frames on average; base_frame ascends and the codes emit where it says
    bf = (torch.arange(M, device=dev, dtype=torch.int64) * F // M).to(torch.int32).repeat(N)
    codes = torch.randint(0, 4, (nframes,), device=dev, generator=gen, dtype=torch.uint8)
    codes.view(N, F)[:, (torch.arange(M, device=dev, dtype=torch.int64) * F // M)] |= 0x80
    rb = torch.arange(N + 1, device=dev, dtype=torch.int64) * M
    rf = torch.arange(N + 1, device=dev, dtype=torch.int64) * F
    decoded = DecodedReads(seq, rb, torch.zeros(N, dtype=torch.int32, device=dev), bf, None, codes, None)
    ids = torch.from_numpy(rng.integers(0, 256, (N, 16)).astype(np.uint8)).to(dev)
    s = codec.stream

    hits = demux.find_patterns(codec, decoded, pats, window=W, stream=s)
    cls = demux.classify(codec, decoded, hits, pats, NB, 3, stream=s)
    cut = demux.trim_reads(codec, decoded, cls.lo, cls.hi, qual=qual, moves=(codes, rf, 5), stream=s)
    torch.cuda.synchronize()

    # checks before any time counts
    seq_host = seq.cpu().numpy()
    sample = sorted(set([0, 1, N // 2, N - 1] + rng.integers(0, N, 8).tolist()))
    good = True
    for r in sample:
        want = host.find_patterns_signal(seq_host[r * M:(r + 1) * M], [0, M], [0], sets.patterns, sets.side, sets.max_dist, W)
        for name, w in zip(("dist", "start", "end"), want):
            good = good and np.array_equal(getattr(hits, name)[r].cpu().numpy().view(np.uint32), w[0])
    say(f"sampled reads' hits equal the host model's: {good}")
    barcode = cls.barcode.cpu().numpy()
    lo, hi = cls.lo.cpu().numpy().astype(np.int64), cls.hi.cpu().numpy().astype(np.int64)
    nhits = int((hits.start != -1).sum().item())
    say(f"barcodes recovered: {int((barcode == planted).sum())} of {N} ({int((planted >= 0).sum())} planted, "
        f"{int((barcode >= 0).sum())} named); reads cut to the planted insert: "
        f"{int(((lo == head_len) & (hi == M - tail_len)).sum())} of {N}; hits: {nhits} of {N * len(sets)} "
        f"({nhits / N:.2f} per read)")
    kept, kept_frames = int(cut.decoded.read_bases[-1].item()), int(cut.read_frames[-1].item())
    say(f"trimmed batch: {kept} of {total} bases, {kept_frames} of {nframes} frames; statuses all 0: "
        f"{bool((cut.decoded.status == 0).all())}")

    tf = timed(lambda: demux.find_patterns(codec, decoded, pats, window=W, stream=s))
    cells = 0
    for side in (0, 1):
        cells += N * min(M, W) * sum(1 for v in sets.side if v == side)
    say(fmt("f find_patterns", tf) + f": {cells / 1e9:.2f} G (pattern, text byte) columns, {mean(tf) * 1e6 / cells * 1e3:.2f} ps each, "
        f"{cells / (mean(tf) * 1e-3) / 1e12:.2f} T columns/s")
    other = demux.find_patterns(plain, decoded, pats, window=W, stream=plain.stream)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(getattr(hits, k), getattr(other, k))) for k in ("dist", "start", "end"))
    del other
    tp = timed(lambda: demux.find_patterns(plain, decoded, pats, window=W, stream=plain.stream))
    short = sum(1 for v in lens if v <= 64)
    say(fmt("p find_patterns, pattern order and two words throughout", tp) + f": its outputs equal f's: {same}; "
        f"{short} of {len(lens)} patterns have at most 64 bytes; f - p = {mean(tf) - mean(tp):+.3f} ms")
    tc = timed(lambda: demux.classify(codec, decoded, hits, pats, NB, 3, stream=s))
    say(fmt("c classify", tc) + f": reads {3 * 4 * N * len(sets) / 1e9:.2f} GB of hits")
    tt = timed(lambda: demux.trim_reads(codec, decoded, cls.lo, cls.hi, qual=qual, moves=(codes, rf, 5), stream=s))
    moved = 2 * (2 * kept + kept_frames + 4 * kept)
    say(fmt("t trim_reads (seq, qual, base_frame, codes)", tt) + f": {moved / 1e9:.2f} GB read and written, "
        f"{moved / (mean(tt) * 1e-3) / 1e9:.0f} GB/s")

    tags = {"bc": cls.barcode, "ts": cut.trim_frames}
    mv = (cut.codes, cut.read_frames, 5)
    bound = bam.bam_bound(N, int(cut.decoded.seq.numel()), 2, int(cut.codes.numel()))
    raw_out = torch.empty(bound, dtype=torch.uint8, device=dev)
    gz_out = torch.empty(bam.bgzf_bound(bound), dtype=torch.uint8, device=dev)

    def records():
        rec = bam.bam_records(codec, cut.decoded, cut.qual, ids, tags, moves=mv, bgzf=False, out=raw_out, stream=s)
        return bgzf.bgzf_deflate(codec, rec.data, rec.written[:1], out=gz_out, stream=s)

    blk = records()
    torch.cuda.synchronize()
    say(f"records of the trimmed batch: file {int(blk.written[1].item())} bytes")
    tr = timed(records)
    say(fmt("r bam_records (raw, moves) + bgzf_deflate of the trimmed batch", tr))
    three = [a + b + c for a, b, c in zip(tf, tc, tt)]
    spread = lambda runs: max(runs) - min(runs)
    longest = max((("find_patterns", mean(tf)), ("classify", mean(tc)), ("trim_reads", mean(tt))), key=lambda kv: kv[1])
    say(f"condition: f + c + t < r: {mean(three) < mean(tr)} (f + c + t {mean(three):.3f} ms, runs' spread {spread(three):.3f}; "
        f"r {mean(tr):.3f} ms, runs' spread {spread(tr):.3f}); the longest of the three is {longest[0]}, {longest[1]:.3f} ms")

    # the host route: the download, then the model on a sample of reads in threads
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    down = seq.cpu().numpy()
    t_down = (time.perf_counter() - t0) * 1e3
    K = min(args.host_reads, N)

    def work(r):
        host.find_patterns_signal(down[r * M:(r + 1) * M], [0, M], [0], sets.patterns, sets.side, sets.max_dist, W)

    th = []
    with ThreadPoolExecutor(args.threads) as pool:
        for _ in range(args.runs):
            t0 = time.perf_counter()
            list(pool.map(work, range(K)))
            th.append((time.perf_counter() - t0) * 1e3)
    say(fmt(f"h host find_patterns_signal of {K} reads in {args.threads} threads", th) + f"; SCALED to {N} reads: "
        f"{mean(th) * N / K / 1e3:.0f} s, behind a download of the bases of {t_down:.0f} ms (measured once); the model is "
        f"numpy code written as the rule reads, not an optimised host search")
    codec.close()
    plain.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
