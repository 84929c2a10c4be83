#!/usr/bin/env python3
"""Mean quality and FASTQ records (fastq.read_qual, fastq.fastq_records) against the torch route and a device copy,
at the bench's shape carried to bases: 100,000 reads of 20,000 frames, of which tools/ctc_timing.py found 32 %
emitting, so 6,400 bases per read; qualities uniform in [33, 83], bases uniform in ACGT, random ids, two tags (the
mean quality as ``qs`` and a channel as ``ch``).  A second, heavy-tailed shape has the same number of bases with one
read holding 4 x 10^6 of them.  One process, HIP events on the caller's stream.

Quantities per shape (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  q   read_qual: reads the qualities once
  f   fastq_records into a buffer of fastq_bound bytes: reads seq and qual once, writes the text once
  c   a device-to-device copy of as many bytes as f writes (so it reads and writes what f does, to within the headers)
  t   the torch route that yields the same bytes: one torch.take over the concatenation of the pre-formatted headers,
      seq, qual and the constant bytes, with an int64 source index per output byte.  The index is built beforehand
      (on the device, from the per-read segments) and is not timed; tools/stitch_timing.py found this form fastest.
  h   the route before these calls, once and for the uniform shape only (it is host work, reported for the README and
      no condition): download seq, qual and the offsets, compute each read's mean quality and format in Python.
The device's text is compared with fastq_records_signal on a sample of reads and with the torch route's bytes in full
before any time counts.  Conditions: (a) f < t by more than the spread of both over their runs; (b) the heavy-tailed
shape's f per output byte is within that spread of the uniform shape's.  The tool prints the verdicts and changes
nothing to make them hold.

    python tools/fastq_timing.py [--reads N] [--bases M] [--long L] [--runs R] [--steps K] [--no-torch] [--no-host] [--out FILE]
"""
import argparse
import os
import sys
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch

    import bench
    from rawnanoporesignalcompression_amd import DecodedReads, PGNanoCodec, _native, fastq

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--bases", type=int, default=6_400, help="bases per read of the uniform shape")
    p.add_argument("--long", type=int, default=4_000_000, help="bases of the heavy-tailed shape's long read")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--no-torch", action="store_true", help="skip the torch route")
    p.add_argument("--no-host", action="store_true", help="skip the host route")
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

    def fmt(name, runs):
        return f"{name} {sum(runs) / len(runs):9.3f} ms (runs " + ", ".join(f"{v:.3f}" for v in runs) + ")"

    spread = lambda runs: max(runs) - min(runs)
    mean = lambda runs: sum(runs) / len(runs)
    N, total = args.reads, args.reads * args.bases
    say(f"fastq_timing: {torch.cuda.get_device_name(0)}, {N} reads, {total} bases, qualities in [33, 83], two tags, "
        f"{args.runs} runs x {args.steps} steps, warmup {args.warmup}"
        + (f", library {os.environ['PGN_LIB']}" if os.environ.get("PGN_LIB") else ""))
    say(f"stream_copy_gbs {bench.stream_copy_gbs(torch):.1f} (read + write bytes of a device-to-device copy)")
    codec = PGNanoCodec(0)
    rng = np.random.default_rng(args.seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (total,), device=dev, generator=gen)]
    qual = torch.randint(33, 84, (total,), device=dev, generator=gen, dtype=torch.uint8)
    ids_host = rng.integers(0, 256, (N, 16)).astype(np.uint8)
    ids = torch.from_numpy(ids_host).to(dev)
    ch_host = rng.integers(1, 3001, N).astype(np.int32)
    ch = torch.from_numpy(ch_host).to(dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    per_byte = {}

    shapes = [("uniform", np.full(N, args.bases, np.int64))]
    if args.long and N > 1 and args.long < total:
        rest = total - args.long
        tail = np.full(N, rest // (N - 1), np.int64)
        tail[:rest % (N - 1)] += 1
        tail[N // 2] = args.long
        tail[-1] += total - int(tail.sum())
        shapes.append(("heavy-tailed", tail))
    for shape, m_host in shapes:
        assert int(m_host.sum()) == total and (m_host > 0).all()
        rb_host = np.concatenate([[0], np.cumsum(m_host)]).astype(np.int64)
        rb = torch.from_numpy(rb_host).to(dev)
        decoded = DecodedReads(seq, rb, status, None, None, None, None)
        say(f"{shape}: reads of {int(m_host.min())} to {int(m_host.max())} bases")
        rq = fastq.read_qual(codec, decoded, qual, stream=codec.stream)
        tags = {"qs": rq.mean_q, "ch": ch}
        out = torch.empty(fastq.fastq_bound(N, total, 2), dtype=torch.uint8, device=dev)
        rec = fastq.fastq_records(codec, decoded, qual, ids, tags, out=out, stream=codec.stream)
        torch.cuda.synchronize()
        off_host = rec.rec_off.cpu().numpy()
        nbytes = int(off_host[-1])
        mq_host = rq.mean_q.cpu().numpy()
        say(f"  text {nbytes} bytes in a buffer of {int(out.numel())}; mean_q {int(mq_host.min())} to {int(mq_host.max())}; "
            f"statuses all 0: {bool((rec.status == 0).all())}")
        # the device's text against the host model on a sample of reads
        sample = sorted(set([0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1] + rng.integers(0, N, 20).tolist()))
        good = True
        for r in sample:
            a, b = int(rb_host[r]), int(rb_host[r + 1])
            want = fastq.fastq_records_signal(ids_host[r:r + 1], seq[a:b].cpu().numpy(), qual[a:b].cpu().numpy(), [0, b - a], [0],
                                              {"qs": mq_host[r:r + 1].view(np.uint32), "ch": ch_host[r:r + 1]})[0]
            good = good and out[int(off_host[r]):int(off_host[r + 1])].cpu().numpy().tobytes() == want
            mq = fastq.read_qual_signal(qual[a:b].cpu().numpy(), [0, b - a], [0], None, q_min=1, skip_bases=60, min_mean_q=0)[0]
            good = good and int(mq[0]) == int(mq_host[r])
        say(f"  {len(sample)} sampled reads' records and mean qualities equal the host models': {good}")

        tq = timed(lambda: fastq.read_qual(codec, decoded, qual, stream=codec.stream))
        say("  " + fmt("q read_qual", tq) + f": reads {total / 1e9:.2f} GB, {total / (mean(tq) * 1e-3) / 1e9:.0f} GB/s")
        tf = timed(lambda: fastq.fastq_records(codec, decoded, qual, ids, tags, out=out, stream=codec.stream))
        moved = 2 * total + nbytes
        say("  " + fmt("f fastq_records", tf) + f": reads {2 * total / 1e9:.2f} GB, writes {nbytes / 1e9:.2f} GB, "
            f"{moved / (mean(tf) * 1e-3) / 1e9:.0f} GB/s moved, {mean(tf) * 1e9 / nbytes:.3f} ps per output byte")
        per_byte[shape] = ([v * 1e9 / nbytes for v in tf])
        tile = _native.PGN_FASTQ_TILE_BYTES
        ntiles = -(-nbytes // tile)
        say(f"  {ntiles - len(np.unique(off_host[:-1] // tile))} of {ntiles} output tiles hold no record's start: they lie "
            "inside one record, format no header and search for no record")
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tc = timed(lambda: dst.copy_(src))
        say("  " + fmt(f"c device copy of {nbytes} bytes", tc) + f": {2 * nbytes / (mean(tc) * 1e-3) / 1e9:.0f} GB/s moved; "
            f"f is {mean(tf) / mean(tc):.2f} x c")
        del src, dst

        if not args.no_torch:
            # headers on the host, the source index on the device: per record the segments header, SEQ, "\n+\n", QUAL, "\n"
            heads = [f"@{uuid.UUID(bytes=ids_host[r].tobytes())}\tqs:i:{int(mq_host[r])}\tch:i:{int(ch_host[r])}\n".encode()
                     for r in range(N)]
            hlen = np.array([len(h) for h in heads], np.int64)
            hoff = np.concatenate([[0], np.cumsum(hlen)])
            H = int(hoff[-1])
            source = torch.cat([torch.from_numpy(np.frombuffer(b"".join(heads), np.uint8).copy()).to(dev), seq, qual,
                                torch.tensor(list(b"\n+\n"), dtype=torch.uint8, device=dev)])
            S0, Q0, C0 = H, H + total, H + 2 * total
            lens = np.stack([hlen, m_host, np.full(N, 3), m_host, np.ones(N, np.int64)], 1).reshape(-1)
            start = np.stack([hoff[:-1], S0 + rb_host[:-1], np.full(N, C0), Q0 + rb_host[:-1], np.full(N, C0)], 1).reshape(-1)
            segoff = np.concatenate([[0], np.cumsum(lens)])[:-1]
            shift = torch.from_numpy((start - segoff).astype(np.int64)).to(dev)
            index = torch.repeat_interleave(shift, torch.from_numpy(lens.astype(np.int64)).to(dev))
            index += torch.arange(nbytes, device=dev)
            took = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            torch.take(source, index, out=took)
            say(f"  the torch route's bytes equal fastq_records': {bool(torch.equal(took, out[:nbytes]))} "
                f"(index {index.numel() * 8 / 1e9:.1f} GB, not timed)")
            tt = timed(lambda: torch.take(source, index, out=took))
            margin = spread(tf) + spread(tt)
            say("  " + fmt("t torch route (one take over headers + seq + qual + constants)", tt))
            say(f"  (a) f < t by more than the spread of both: {mean(tt) - mean(tf) > margin} (f {mean(tf):.3f} ms, t "
                f"{mean(tt):.3f} ms; spreads {margin:.3f} ms)")
            del source, index, took, shift
            torch.cuda.empty_cache()

        if not args.no_host and shape == "uniform":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s_h, q_h, rb_h = seq.cpu().numpy(), qual.cpu().numpy(), rb.cpu().numpy()
            t1 = time.perf_counter()
            table = fastq.err_table().astype(np.float64)
            parts = []
            for r in range(N):
                a, b = int(rb_h[r]), int(rb_h[r + 1])
                qs = q_h[a:b]
                e = table[np.clip(qs[60:] if b - a > 60 else qs, 33, 126) - 33].mean() / 2.0 ** 32
                parts.append(b"@%s\tqs:i:%d\tch:i:%d\n%s\n+\n%s\n" % (str(uuid.UUID(bytes=ids_host[r].tobytes())).encode(),
                                                                  int(round(-10 * np.log10(e))), int(ch_host[r]),
                                                                  s_h[a:b].tobytes(), qs.tobytes()))
            text = b"".join(parts)
            t2 = time.perf_counter()
            say(f"  h host route, once: download {(t1 - t0) * 1e3:.0f} ms, mean quality and formatting in Python "
                f"{(t2 - t1) * 1e3:.0f} ms, {len(text)} bytes")
            del parts, text
        del out, rec, rq

    if len(per_byte) == 2:
        u, h = per_byte["uniform"], per_byte["heavy-tailed"]
        margin = spread(u) + spread(h)
        say(f"(b) heavy-tailed per output byte within the spread of both of uniform's: {abs(mean(h) - mean(u)) <= margin} "
            f"(uniform {mean(u):.4f} ps, heavy-tailed {mean(h):.4f} ps, {100 * (mean(h) / mean(u) - 1):+.2f} %; spreads "
            f"{margin:.4f} ps)")
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
