#!/usr/bin/env python3
"""Selection of long reads: read_stats (and segment_reads) on reads far longer than a batch's share, where
one workgroup per read leaves the device idle and the split selection (PGNanoCodec.set_select_split)
spreads a read's parts over it.  One process times one tree, HIP events around each call; a figure is the
mean of `--steps` calls after `--warmup`.  The tree under test is `--tree` (default: this one), so the same
tool times a checkout of the parent commit, which has no split: run the two interleaved, parent first, and
compare the lines.  Legs (`--legs`, comma separated):

  single   one read alone of 10^5, 3x10^5, 10^6, 3x10^6 and 10^7 samples, quantile and med/MAD
  off      the same with max_split_reads = 0 (this tree's one-workgroup path; not a stand-in for the parent)
  parts    one read of 10^6 and of 10^7 samples under part_samples 16,384 .. 262,144 (split above one part)
  lengths  one read of 32,768 .. 2,097,152 samples with the split forced on (split_min_samples = part_samples
           = `--part`) against the split off: where the split stops paying for a lone read
  ragged   2,000 reads with lengths log-uniform in [2,000, 5x10^6] and one of 2x10^7 (seed 1): read_stats in
           both modes and segment_reads (L 10,000, V 500, the usual trim, float16), with the split counters
  uniform  100,000 synthetic reads of 100,000 samples, where no read is split and the plan is pure cost:
           read_stats in both modes (uniform_off: the same with max_split_reads = 0)

Samples are Gaussian, sd 60 around 500 counts, as int16.

    python tools/select_split_timing.py [--tree DIR] [--legs single,ragged] [--label NAME] [--out FILE]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTILE = dict(mode="quantile", p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, spread_floor=1.0)
MEDMAD = dict(mode="medmad", p=(0.2, 0.9), centre_mult=0.51, spread_mult=1.4826, spread_floor=1.0)
MODES = {"quantile": QUANTILE, "medmad": MEDMAD}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--tree", default=HERE, help="the checkout whose package is timed")
    p.add_argument("--legs", default="single,off,parts,lengths,ragged")
    p.add_argument("--label", default=None)
    p.add_argument("--part", type=int, default=None, help="part_samples of the lengths and ragged legs (default: the context's)")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    from rawnanoporesignalcompression_amd import PGNanoCodec

    dev = torch.device("cuda", 0)
    label = args.label or os.path.basename(os.path.abspath(args.tree))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
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
        return sum(ms) / len(ms), min(ms)

    codec = PGNanoCodec(0)
    can_split = hasattr(codec, "set_select_split")
    defaults = codec.select_split if can_split else None
    say(f"select_split_timing [{label}]: {torch.cuda.get_device_name(0)}, {args.steps} steps, warmup {args.warmup}, "
        f"select_split {defaults if can_split else 'not in this tree'}")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def signal(n):
        return (torch.randn(n, device=dev, generator=gen) * 60 + 500).round().to(torch.int16)

    def one_read(x, prm):
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        cnt = torch.full((1,), x.numel(), dtype=torch.int64, device=dev)
        return timed(lambda: codec.read_stats(x, off, cnt, **prm))

    def counts_text():
        return f" {codec.select_split_counts()}" if can_split else ""

    legs = args.legs.split(",")
    big = signal(10_000_000)
    for leg in ("single", "off"):
        if leg not in legs or (leg == "off" and not can_split):
            continue
        if can_split:
            codec.set_select_split(*(defaults if leg == "single" else defaults[:2] + (0,)))
        for n in (100_000, 300_000, 1_000_000, 3_000_000, 10_000_000):
            for name, prm in MODES.items():
                mean, best = one_read(big[:n], prm)
                say(f"[{label}] {leg:7s} n {n:>10,} {name:8s} {mean:8.3f} ms (min {best:.3f}){counts_text()}")
    if "parts" in legs and can_split:
        for n in (1_000_000, 10_000_000):
            for part in (16_384, 32_768, 65_536, 131_072, 262_144):
                codec.set_select_split(part, part, defaults[2] or 1024)
                for name, prm in MODES.items():
                    mean, best = one_read(big[:n], prm)
                    say(f"[{label}] parts   n {n:>10,} part_samples {part:>7,} {name:8s} {mean:8.3f} ms (min {best:.3f}){counts_text()}")
    if "lengths" in legs and can_split:
        part = args.part or defaults[1]
        for n in (32_768, 49_152, 65_536, 98_304, 131_072, 196_608, 262_144, 524_288, 1_048_576, 2_097_152):
            if n <= part:
                continue
            for name, prm in MODES.items():
                codec.set_select_split(part, part, defaults[2] or 1024)
                on = one_read(big[:n], prm)
                codec.set_select_split(part, part, 0)
                off = one_read(big[:n], prm)
                say(f"[{label}] lengths n {n:>10,} part_samples {part:,} {name:8s} split {on[0]:7.3f} ms (min {on[1]:.3f}), "
                    f"one workgroup {off[0]:7.3f} ms (min {off[1]:.3f})")
    if can_split:
        codec.set_select_split(*defaults)
    del big
    if "ragged" in legs:
        if can_split and args.part:
            codec.set_select_split(max(defaults[0], args.part), args.part, defaults[2])
            say(f"[{label}] ragged under select_split {codec.select_split}")
        rng = np.random.default_rng(1)
        lens = np.exp(rng.uniform(np.log(2_000), np.log(5_000_000), 2_000)).astype(np.int64)
        lens = np.concatenate([lens, [20_000_000]])
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        x = signal(int(lens.sum()))
        d_off, d_cnt = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
        say(f"[{label}] ragged: {lens.size} reads, {int(lens.sum()):,} samples, longest {int(lens.max()):,}, median {int(np.median(lens)):,}")
        for name, prm in MODES.items():
            mean, best = timed(lambda: codec.read_stats(x, d_off, d_cnt, **prm))
            say(f"[{label}] ragged  read_stats {name:8s} {mean:8.3f} ms (min {best:.3f}){counts_text()}")
        L, V = 10_000, 500
        cap = int(np.where(lens > L, (np.maximum(lens - L, 0) + (L - V) - 1) // (L - V) + 1, 1).sum())
        out = torch.empty((cap, L), dtype=torch.float16, device=dev)
        mean, best = timed(lambda: codec.segment_reads(x, d_off, d_cnt, length=L, overlap=V, trim=True, dtype=torch.float16,
                                                       capacity=cap, out=out, **QUANTILE))
        say(f"[{label}] ragged  segment_reads quantile float16 L {L} V {V} usual trim {mean:8.3f} ms (min {best:.3f}), "
            f"{cap} rows{counts_text()}")
    for leg in ("uniform", "uniform_off"):
        if leg not in legs or (leg == "uniform_off" and not can_split):
            continue
        if can_split:
            codec.set_select_split(*(defaults if leg == "uniform" else defaults[:2] + (0,)))
        R, n = 100_000, 100_000
        x, offs, _ = codec.synth_reads(R, n, seed=42)
        d_off = offs.to(torch.int64).contiguous()
        d_cnt = torch.full((R,), n, dtype=torch.int64, device=dev)
        for name, prm in MODES.items():
            mean, best = timed(lambda: codec.read_stats(x, d_off, d_cnt, **prm))
            say(f"[{label}] {leg:11s} {R:,} reads x {n:,} samples read_stats {name:8s} {mean:8.3f} ms (min {best:.3f}){counts_text()}")
        del x
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
