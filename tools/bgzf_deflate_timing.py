#!/usr/bin/env python3
"""BGZF deflate (bgzf.bgzf_deflate) on the raw BAM records of tools/bam_timing.py's batch and on the FASTQ text of
tools/fastq_timing.py's uniform shape, against the stored BGZF call, a device copy and the host route a user would
otherwise take.  The batch is bam_timing's as that tool makes it: 100,000 reads of 6,400 bases (qualities uniform
in [33, 83]: 51 values, 5.67 bits each; bases uniform in ACGT: the 16 packed values, 4 bits a byte; random ids, two
tags) plus 16,000 frames per read whose codes emit at 40 % (a move-table byte holds 0.97 bits).  One process, HIP
events on the codec's stream.

Quantities per stream (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  d    the device route: the record call (raw layout) and bgzf_deflate behind it, with no host wait between them (the
       stream's length is read on the device)
  z    bgzf_deflate alone
  p, s the plan kernel alone and the plan and scan kernels (PGN_BGZF_KERNELS=plan | scan, further contexts of the
       same process); the pack kernel is z - s
  b    the stored route: bam_records(bgzf=True) (BAM only)
  c    a device-to-device copy of as many bytes as the stored form has
  h    the host route on the same bytes: the download of the raw stream, then zlib Z_HUFFMAN_ONLY (raw deflate, level
       1) of every 65,280-byte payload with zlib.crc32 and the block's frame, in 16 threads
Before any time counts, sampled blocks of the device's file are compared with deflate_block_signal bit for bit and
inflated with zlib, the file's length with blk_off, and the last block with the stream's end.  For the record only:
the file's bytes against the stored form's and, on a sample of blocks, against zlib levels 1 and 6 and
Z_HUFFMAN_ONLY.  Condition: d < h by more than the two routes' combined run-to-run spread.  The tool prints the
verdict and changes nothing to make it hold.

    python tools/bgzf_deflate_timing.py [--reads N] [--bases M] [--frames F] [--runs R] [--steps K] [--out FILE]
"""
import argparse
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch

    import bench
    from rawnanoporesignalcompression_amd import DecodedReads, PGNanoCodec, _native, bam, bgzf, fastq

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--bases", type=int, default=6_400)
    p.add_argument("--frames", type=int, default=16_000)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--sample", type=int, default=24, help="blocks compared with the model and with zlib's levels")
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
    spread = lambda runs: max(runs) - min(runs)
    fmt = lambda name, runs: f"{name} {mean(runs):9.3f} ms (runs " + ", ".join(f"{v:.3f}" for v in runs) + ")"
    N, M, F = args.reads, args.bases, args.frames
    total, nframes = N * M, N * F
    B = _native.PGN_BGZF_BLOCK_BYTES
    say(f"bgzf_deflate_timing: {torch.cuda.get_device_name(0)}, {N} reads of {M} bases and {F} frames, two tags, "
        f"{args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    say(f"stream_copy_gbs {bench.stream_copy_gbs(torch):.1f} (read + write bytes of a device-to-device copy)")
    codec = PGNanoCodec(0)
    partial = {}
    for kernels in ("plan", "scan"):
        os.environ["PGN_BGZF_KERNELS"] = kernels
        partial[kernels] = PGNanoCodec(0)
    del os.environ["PGN_BGZF_KERNELS"]
    rng = np.random.default_rng(args.seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (total,), device=dev, generator=gen)]
    qual = torch.randint(33, 84, (total,), device=dev, generator=gen, dtype=torch.uint8)
    codes = torch.randint(0, 4, (nframes,), device=dev, generator=gen, dtype=torch.uint8)
    codes |= (torch.rand(nframes, device=dev, generator=gen) < 0.4).to(torch.uint8) << 7
    ids = torch.from_numpy(rng.integers(0, 256, (N, 16)).astype(np.uint8)).to(dev)
    tags = {"qs": torch.from_numpy(rng.integers(1, 51, N).astype(np.int32)).to(dev),
            "ch": torch.from_numpy(rng.integers(1, 3001, N).astype(np.int32)).to(dev)}
    rb = torch.arange(N + 1, device=dev, dtype=torch.int64) * M
    rf = torch.arange(N + 1, device=dev, dtype=torch.int64) * F
    decoded = DecodedReads(seq, rb, torch.zeros(N, dtype=torch.int32, device=dev), None, None, None, None)
    say("qualities uniform in [33, 83] (51 values), bases uniform in ACGT, 40 % of the frames emit")

    def host_block(view, n):
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        body = z.compress(view) + z.flush()
        if len(body) >= n + 5:
            body = struct.pack("<BHH", 1, n, n ^ 0xFFFF) + bytes(view)
        return b"".join((bgzf_head, struct.pack("<H", len(body) + 25), body, struct.pack("<II", zlib.crc32(view), n)))

    bgzf_head = bytes.fromhex("1f8b08040000000000ff060042430200")

    def measure(label, raw, length, produce, stored_call):
        """raw: the device buffer the records are in; length(): the one-element device tensor with their bytes, of
        the last record call;
        produce(): the record call into raw."""
        cap = int(raw.numel())
        out = torch.empty(bgzf.bgzf_bound(cap), dtype=torch.uint8, device=dev)
        deflate = lambda c=codec: bgzf.bgzf_deflate(c, raw, length(), out=out, stream=c.stream)
        produce()
        blocks = deflate()
        torch.cuda.synchronize()
        W = int(length().item())
        consumed, nfile = (int(v) for v in blocks.written.cpu().numpy())
        off = blocks.blk_off.cpu().numpy()
        nblocks = -(-W // B)
        stored = W + 31 * nblocks
        say(f"{label}: stream {W} bytes in {nblocks} blocks of a buffer of {cap}; file {nfile} bytes, "
            f"{nfile / stored:.4f} of the stored form's {stored}; consumed all: {consumed == W}; "
            f"blk_off ends at the file's length: {int(off[nblocks]) == nfile == int(off[-1])}")
        sample = sorted(set([0, 1, nblocks - 1] + rng.integers(0, nblocks, args.sample).tolist()))
        good, sizes = True, {"device": 0, "huffman": 0, "level1": 0, "level6": 0, "payload": 0}
        for k in sample:
            payload = raw[k * B:min((k + 1) * B, W)].cpu().numpy().tobytes()
            blk = out[int(off[k]):int(off[k + 1])].cpu().numpy().tobytes()
            body = blk[18:-8]
            z = zlib.decompressobj(-15)
            good = good and blk[:16] == bgzf_head and struct.unpack_from("<H", blk, 16)[0] == len(blk) - 1
            good = good and body == bgzf.deflate_block_signal(payload) and z.decompress(body) == payload and z.eof
            good = good and struct.unpack_from("<II", blk, len(blk) - 8) == (zlib.crc32(payload), len(payload))
            sizes["device"] += len(body)
            sizes["payload"] += len(payload)
            for key, level, strategy in (("huffman", 1, zlib.Z_HUFFMAN_ONLY), ("level1", 1, zlib.Z_DEFAULT_STRATEGY),
                                         ("level6", 6, zlib.Z_DEFAULT_STRATEGY)):
                zc = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
                sizes[key] += len(zc.compress(payload) + zc.flush())
        say(f"  {len(sample)} sampled blocks equal deflate_block_signal bit for bit, inflate with zlib to their payloads "
            f"and carry their CRC-32 and lengths: {good}")
        say(f"  for the record, deflate bytes of those blocks ({sizes['payload']} payload bytes): device {sizes['device']}, "
            f"zlib Z_HUFFMAN_ONLY {sizes['huffman']}, level 1 {sizes['level1']}, level 6 {sizes['level6']} "
            f"(device / payload {sizes['device'] / sizes['payload']:.4f}, level 6 / payload {sizes['level6'] / sizes['payload']:.4f})")

        def route():
            produce()
            deflate()

        td = timed(route)
        say("  " + fmt("d records raw + bgzf_deflate", td))
        tz = timed(deflate)
        say("  " + fmt("z bgzf_deflate alone", tz) + f": reads {W / 1e9:.2f} GB twice, writes {nfile / 1e9:.2f} GB, "
            f"{mean(tz) * 1e9 / W:.3f} ps per stream byte, {W / (mean(tz) * 1e-3) / 1e9:.0f} GB/s of stream")
        tp = timed(lambda: deflate(partial["plan"]))
        ts = timed(lambda: deflate(partial["scan"]))
        say("  " + fmt("p the plan kernel alone", tp) + f": {mean(tp) * 1e6 / nblocks:.2f} ns per block over the device")
        say("  " + fmt("s the plan and scan kernels", ts) + f": the scan {mean(ts) - mean(tp):+.3f} ms, the pack kernel "
            f"z - s = {mean(tz) - mean(ts):.3f} ms")
        deflate()                                            # the full call's bytes again behind the partial ones
        if stored_call is not None:
            tb = timed(stored_call)
            say("  " + fmt("b the record call in stored BGZF blocks", tb) + f": d is {mean(td) / mean(tb):.2f} x b for "
                f"{nfile / stored:.3f} of its bytes")
        src, dst = torch.empty(stored, dtype=torch.uint8, device=dev), torch.empty(stored, dtype=torch.uint8, device=dev)
        tc = timed(lambda: dst.copy_(src))
        say("  " + fmt(f"c device copy of {stored} bytes", tc) + f": z is {mean(tz) / mean(tc):.2f} x c")
        del src, dst

        # the host route on the same bytes
        produce()
        torch.cuda.synchronize()
        th, tdown = [], []
        per = -(-nblocks // args.threads)
        pieces = [None] * args.threads
        with ThreadPoolExecutor(args.threads) as pool:
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = raw[:W].cpu().numpy()
                t1 = time.perf_counter()
                view = memoryview(host)

                def work(i):
                    pieces[i] = b"".join(host_block(view[k * B:min((k + 1) * B, W)], min(B, W - k * B))
                                         for k in range(i * per, min((i + 1) * per, nblocks)))

                list(pool.map(work, range(args.threads)))
                t2 = time.perf_counter()
                tdown.append((t1 - t0) * 1e3)
                th.append((t2 - t0) * 1e3)
        nhost = sum(len(x) for x in pieces)
        say("  " + fmt(f"h host route: download, zlib Z_HUFFMAN_ONLY and crc32 per block in {args.threads} threads", th)
            + f"; of that the download " + ", ".join(f"{v:.0f}" for v in tdown) + f" ms; its file has {nhost} bytes, "
            f"the device's {nfile} ({nfile / nhost:.4f})")
        gap, both = mean(th) - mean(td), spread(th) + spread(td)
        say(f"  condition: d < h by more than the combined spread: {gap > both} (h - d = {gap:.3f} ms, spreads "
            f"{spread(td):.3f} + {spread(th):.3f} ms; h / d = {mean(th) / mean(td):.1f})")
        del out, host, pieces

    # the BAM records with the move table
    mv = (codes, rf, 5)
    bound = bam.bam_bound(N, total, 2, nframes)
    raw = torch.empty(bound, dtype=torch.uint8, device=dev)
    holder = {}

    def bam_raw():
        holder["rec"] = bam.bam_records(codec, decoded, qual, ids, tags, moves=mv, bgzf=False, out=raw, stream=codec.stream)

    bam_raw()
    stored_out = torch.empty(bam.bgzf_bound(bound), dtype=torch.uint8, device=dev)
    measure("BAM records with the move table", raw, lambda: holder["rec"].written[:1], bam_raw,
            lambda: bam.bam_records(codec, decoded, qual, ids, tags, moves=mv, bgzf=True, out=stored_out, stream=codec.stream))
    del raw, stored_out, codes
    holder.clear()

    # the FASTQ text of the uniform shape, the mean quality as qs
    rq = fastq.read_qual(codec, decoded, qual, stream=codec.stream)
    ftags = {"qs": rq.mean_q, "ch": tags["ch"]}
    text = torch.empty(fastq.fastq_bound(N, total, 2), dtype=torch.uint8, device=dev)

    def fastq_text():
        holder["rec"] = fastq.fastq_records(codec, decoded, qual, ids, ftags, out=text, stream=codec.stream)

    fastq_text()
    measure("FASTQ text", text, lambda: holder["rec"].rec_off[-1:], fastq_text, None)
    codec.close()
    for c in partial.values():
        c.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
