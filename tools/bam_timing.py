#!/usr/bin/env python3
"""BAM records (bam.bam_records) against a device copy, fastq_records and the host's BGZF framing, at the FASTQ
timing's shape: 100,000 reads of 6,400 bases (qualities uniform in [33, 83], bases uniform in ACGT, random ids, two
tags) plus 16,000 frames per read whose codes emit at 40 %.  One process, HIP events on the codec's stream.

Quantities (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  r    bam_records, raw layout, without and with the move table
  b    bam_records, BGZF layout (the CRC fused into the writer), without and with the move table
  s    the same with the other CRC placement (PGN_BAM_CRC=split: the writer stores the payloads, a second kernel reads
       each back, checksums it and writes the block's 31 bytes), on a second context of the same process
  c    a device-to-device copy of as many bytes as b writes
  f    fastq_records on the same reads
  h    the host route's framing step alone on the same bytes: the raw records downloaded beforehand (not timed), then
       zlib.crc32 of every 65,280-byte payload in 16 threads, each block's 23 + 8 bytes written in place
Before any time counts, sampled reads' records are compared with bam_records_signal, sampled blocks' CRC fields with
zlib.crc32, and the two placements' bytes with each other in full.  Condition: b (with moves) < h.  The tool prints
the verdict and changes nothing to make it hold.

    python tools/bam_timing.py [--reads N] [--bases M] [--frames F] [--runs R] [--steps K] [--out FILE]
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
    from rawnanoporesignalcompression_amd import DecodedReads, PGNanoCodec, _native, bam, fastq

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
    N, M, F = args.reads, args.bases, args.frames
    total, nframes = N * M, N * F
    say(f"bam_timing: {torch.cuda.get_device_name(0)}, {N} reads of {M} bases and {F} frames, two tags, "
        f"{args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    say(f"stream_copy_gbs {bench.stream_copy_gbs(torch):.1f} (read + write bytes of a device-to-device copy)")
    fused = PGNanoCodec(0)
    os.environ["PGN_BAM_CRC"] = "split"
    split = PGNanoCodec(0)
    del os.environ["PGN_BAM_CRC"]
    rng = np.random.default_rng(args.seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (total,), device=dev, generator=gen)]
    qual = torch.randint(33, 84, (total,), device=dev, generator=gen, dtype=torch.uint8)
    codes = torch.randint(0, 4, (nframes,), device=dev, generator=gen, dtype=torch.uint8)
    codes |= (torch.rand(nframes, device=dev, generator=gen) < 0.4).to(torch.uint8) << 7
    ids_host = rng.integers(0, 256, (N, 16)).astype(np.uint8)
    ids = torch.from_numpy(ids_host).to(dev)
    qs_host, ch_host = rng.integers(1, 51, N).astype(np.int32), rng.integers(1, 3001, N).astype(np.int32)
    tags = {"qs": torch.from_numpy(qs_host).to(dev), "ch": torch.from_numpy(ch_host).to(dev)}
    rb = torch.arange(N + 1, device=dev, dtype=torch.int64) * M
    rf = torch.arange(N + 1, device=dev, dtype=torch.int64) * F
    decoded = DecodedReads(seq, rb, torch.zeros(N, dtype=torch.int32, device=dev), None, None, None, None)
    mv = (codes, rf, 5)
    B = _native.PGN_BGZF_BLOCK_BYTES

    results = {}
    for label, moves in (("without moves", None), ("with moves", mv)):
        bound = bam.bam_bound(N, total, 2, nframes if moves else None)
        out = torch.empty(bam.bgzf_bound(bound), dtype=torch.uint8, device=dev)
        out2 = torch.empty_like(out)
        call = lambda codec, bgzf, o=out: bam.bam_records(codec, decoded, qual, ids, tags, moves=moves, bgzf=bgzf, out=o,
                                                          stream=codec.stream)
        rec = call(fused, True)
        rec2 = call(split, True, out2)
        torch.cuda.synchronize()
        W, nfile = (int(v) for v in rec.written.cpu().numpy())
        same = bool(torch.equal(out[:nfile], out2[:nfile])) and int(rec2.written[1].item()) == nfile
        say(f"{label}: stream {W} bytes, file {nfile} bytes in {-(-W // B)} blocks; statuses all 0: "
            f"{bool((rec.status == 0).all())}; the two CRC placements' bytes are equal: {same}")
        del out2, rec2
        good = True
        for k in sorted(set([0, 1, -(-W // B) - 1] + rng.integers(0, -(-W // B), 20).tolist())):
            blk = out[k * (B + 31):k * (B + 31) + min(B, W - k * B) + 31].cpu().numpy().tobytes()
            n = len(blk) - 31
            good = good and struct.unpack_from("<II", blk, 23 + n) == (zlib.crc32(blk[23:23 + n]), n)
            good = good and struct.unpack_from("<HBHH", blk, 16) == (n + 30, 1, n, n ^ 0xFFFF)
        say(f"  sampled blocks' BSIZE, lengths and CRC-32 equal zlib's: {good}")
        raw_rec = call(fused, False)
        torch.cuda.synchronize()
        off_host = raw_rec.rec_off.cpu().numpy()
        good = True
        for r in sorted(set([0, 1, N // 2, N - 1] + rng.integers(0, N, 12).tolist())):
            a, b = r * M, (r + 1) * M
            want = bam.bam_records_signal(
                ids_host[r:r + 1], seq[a:b].cpu().numpy(), qual[a:b].cpu().numpy(), [0, M], [0],
                {"qs": qs_host[r:r + 1], "ch": ch_host[r:r + 1]},
                moves=(codes[r * F:(r + 1) * F].cpu().numpy(), [0, F], 5) if moves else None)[0]
            good = good and out[int(off_host[r]):int(off_host[r + 1])].cpu().numpy().tobytes() == want
        say(f"  sampled reads' records equal the host model's: {good}")

        read_bytes = 2 * total + (nframes if moves else 0)
        for key, name, codec, bgzf in (("r", "r bam_records raw", fused, False), ("b", "b bam_records BGZF, CRC fused", fused, True),
                                       ("s", "s bam_records BGZF, CRC in a second kernel", split, True)):
            t = timed(lambda: call(codec, bgzf))
            wrote = nfile if bgzf else W
            moved = read_bytes + wrote + (W if key == "s" else 0)
            say("  " + fmt(name, t) + f": reads {read_bytes / 1e9:.2f} GB, writes {wrote / 1e9:.2f} GB, "
                f"{moved / (mean(t) * 1e-3) / 1e9:.0f} GB/s moved, {mean(t) * 1e9 / wrote:.3f} ps per output byte")
            results[(key, label)] = t
        say(f"  the second kernel reads the {W / 1e9:.2f} GB of payloads back: s - b = "
            f"{mean(results[('s', label)]) - mean(results[('b', label)]):+.3f} ms, b - r = "
            f"{mean(results[('b', label)]) - mean(results[('r', label)]):+.3f} ms")
        src, dst = torch.empty(nfile, dtype=torch.uint8, device=dev), torch.empty(nfile, dtype=torch.uint8, device=dev)
        tc = timed(lambda: dst.copy_(src))
        say("  " + fmt(f"c device copy of {nfile} bytes", tc) + f": {2 * nfile / (mean(tc) * 1e-3) / 1e9:.0f} GB/s moved; "
            f"b is {mean(results[('b', label)]) / mean(tc):.2f} x c")
        del src, dst

        if moves:
            # the host route's framing step on the same bytes
            call(fused, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            raw_host = out[:W].cpu().numpy()
            t_down = time.perf_counter() - t0
            nblocks = -(-W // B)
            frames = np.zeros((nblocks, 31), np.uint8)
            head = bytes.fromhex("1f8b08040000000000ff060042430200")

            def work(lo, hi):
                view = memoryview(raw_host)
                for k in range(lo, hi):
                    n = min(B, W - k * B)
                    crc = zlib.crc32(view[k * B:k * B + n])
                    frames[k] = np.frombuffer(head + struct.pack("<HBHHII", n + 30, 1, n, n ^ 0xFFFF, crc, n), np.uint8)

            th = []
            per = -(-nblocks // args.threads)
            with ThreadPoolExecutor(args.threads) as pool:
                for _ in range(args.runs):
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: work(i * per, min((i + 1) * per, nblocks)), range(args.threads)))
                    th.append((time.perf_counter() - t0) * 1e3)
            call(fused, True)
            torch.cuda.synchronize()
            dev_frames = torch.stack([out[k * (B + 31):k * (B + 31) + 23] for k in (0, nblocks // 2)]).cpu().numpy()
            ok = all(np.array_equal(dev_frames[i], frames[k][:23]) for i, k in enumerate((0, nblocks // 2)))
            tb = results[("b", label)]
            say("  " + fmt(f"h host framing of {W} downloaded bytes, zlib.crc32 in {args.threads} threads", th)
                + f"; its headers equal the device's: {ok}; the download before it took {t_down * 1e3:.0f} ms, not counted")
            say(f"  condition: b < h: {mean(tb) < min(th)} (b {mean(tb):.3f} ms, h {mean(th):.3f} ms, its fastest run "
                f"{min(th):.3f} ms; h / b = {mean(th) / mean(tb):.1f})")
            del raw_host
        del out, rec, raw_rec

    fq_out = torch.empty(fastq.fastq_bound(N, total, 2), dtype=torch.uint8, device=dev)
    tf = timed(lambda: fastq.fastq_records(fused, decoded, qual, ids, tags, out=fq_out, stream=fused.stream))
    nb = int(fastq.fastq_records(fused, decoded, qual, ids, tags, out=fq_out, stream=fused.stream).rec_off[-1].item())
    say(fmt("f fastq_records on the same reads", tf) + f": writes {nb / 1e9:.2f} GB, {mean(tf) * 1e9 / nb:.3f} ps per output byte")
    fused.close()
    split.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
