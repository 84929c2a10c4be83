#!/usr/bin/env python3
"""Decode to the calibrated signal: the fused output of decompress_batch_pa against a separate
elementwise pass over the decoded int16 tensor, at the bench's shape (100,000 chunks x 100,000
samples of C5, blobs from synth_reads + compress_batch), timed with HIP events on the caller's stream,
bench.py's warm-up and step counts.

Legs (all in this one process, on the same blobs):
  a   decompress_batch (int16)
  b   a, then ((out.view(N, L).float() + off[:, None]) * scale[:, None])
  b'  b with .half() appended
  c   decompress_batch_pa(dtype=float32)
  d   decompress_batch_pa(dtype=float16)
and one line for VBZ at the same shape (a, c, d).  The claims under test are c < b and d < b'; the
tool prints both verdicts and changes nothing to make them hold.

    python tools/decode_pa_timing.py [--chunks N] [--samples L] [--out profiles/decode_pa_timing.log]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import torch

    import bench
    from rawnanoporesignalcompression_amd import PGNanoCodec, VBZCodec

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--chunks", type=int, default=100_000)
    p.add_argument("--samples", type=int, default=bdef.samples)
    p.add_argument("--steps", type=int, default=bdef.steps)
    p.add_argument("--warmup", type=int, default=bdef.warmup)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    N, L = args.chunks, args.samples
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    idx = torch.arange(N, dtype=torch.float64, device=dev)
    off = (-243.37 + 0.61 * (idx % 512)).to(torch.float32)  # per chunk, as a read's calibration would be
    scale = (0.17553 * (1 + (idx % 257) / 257)).to(torch.float32)

    def timed(fn):
        """Mean and spread (ms) of fn over the steps, HIP events on the current stream."""
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
        return sum(ms) / len(ms), min(ms), max(ms)

    def fmt(name, t):
        return f"{name} {t[0]:8.2f} ms (min {t[1]:.2f}, max {t[2]:.2f})"

    def run(codec, label, legs_b):
        samples, offs, counts = codec.synth_reads(N, L, seed=args.seed)
        enc = codec.compress_batch(samples, offs, counts, stream=codec.stream)
        torch.cuda.synchronize()
        assert bool((enc.status == 0).all().item())
        del samples
        i16 = torch.empty(N * L, dtype=torch.int16, device=dev)
        fused = {"f32": torch.empty(N * L, dtype=torch.float32, device=dev),
                 "f16": torch.empty(N * L, dtype=torch.float16, device=dev)}
        blob = (enc.blobs, enc.offsets, enc.sizes, counts)

        def leg_a():
            return codec.decompress_batch(*blob, out=i16, out_offsets=offs, stream=codec.stream)[0]

        def leg_b():
            return (leg_a().view(N, L).float() + off[:, None]) * scale[:, None]

        def leg_b2():
            return ((leg_a().view(N, L).float() + off[:, None]) * scale[:, None]).half()

        def leg_c():
            return codec.decompress_batch_pa(*blob, off, scale, dtype=torch.float32, out=fused["f32"], out_offsets=offs,
                                             stream=codec.stream)

        def leg_d():
            return codec.decompress_batch_pa(*blob, off, scale, dtype=torch.float16, out=fused["f16"], out_offsets=offs,
                                             stream=codec.stream)

        # the fused outputs are the separate pass's, bit for bit (checked once, on the first chunks)
        k = min(N, 256)
        want = ((leg_a()[:k * L].view(k, L).float() + off[:k, None]) * scale[:k, None]).reshape(-1)
        st = leg_c()[2]
        leg_d()
        torch.cuda.synchronize()
        assert bool((st == 0).all().item())
        assert torch.equal(fused["f32"][:k * L].view(torch.int32), want.view(torch.int32))
        assert torch.equal(fused["f16"][:k * L].view(torch.int16), want.half().view(torch.int16))
        del want
        torch.cuda.empty_cache()
        ta, tc, td = timed(leg_a), timed(leg_c), timed(leg_d)
        say(f"{label} {N} x {L}: " + "; ".join([fmt("a int16", ta), fmt("c fused f32", tc), fmt("d fused f16", td)]))
        fused.clear()  # the separate pass's temporaries take their place
        torch.cuda.empty_cache()
        if legs_b:
            tb = timed(leg_b)
            torch.cuda.empty_cache()
            tb2 = timed(leg_b2)
            torch.cuda.empty_cache()
            say(f"{label} {N} x {L}: " + "; ".join([fmt("b int16 + torch f32 pass", tb), fmt("b' ... + .half()", tb2)]))
            say(f"{label} c < b: {tc[0] < tb[0]} ({tc[0]:.2f} vs {tb[0]:.2f} ms);  d < b': {td[0] < tb2[0]} "
                f"({td[0]:.2f} vs {tb2[0]:.2f} ms)")

    say(f"decode_pa_timing: {torch.cuda.get_device_name(0)}, steps {args.steps}, warmup {args.warmup}")
    c5 = PGNanoCodec(0)
    run(c5, "C5 ", True)
    c5.close()
    torch.cuda.empty_cache()
    vbz = VBZCodec(0)
    run(vbz, "VBZ", False)
    vbz.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
