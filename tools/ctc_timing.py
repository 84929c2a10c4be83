#!/usr/bin/env python3
"""Stitched frames to bases: ctc_decode and collapse_codes against the torch route, at the shape derived from
the bench's (100,000 reads x 100,000 samples at a model stride of 5: 20,000 frames per read, C = 5 float16
scores per frame), one process, HIP events on the caller's stream.

The scores are made on the device: label runs whose lengths are geometric with a mean of 2.5 frames (a
nanopore base lasts about a dozen samples), a fifth of the runs blank; every class of a frame gets a value in
[-1, 0) and the run's label 2 more, so every frame has a distinct winner.  If the scores and the torch route's
intermediates (int64 labels and an int64 running sum over all frames) do not fit the device together, or a
torch op refuses that many elements, the number of reads is halved until they do, for all three quantities
alike, and the log says which ran.

Quantities (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  d   ctc_decode with all outputs (seq, base_frame, base_score, read_bases, status); its bytes read and written
      over that time, beside stream_copy_gbs measured in this process
  c   collapse_codes alone on the codes d leaves
  t   the route without these calls: frames.argmax(1); the emit mask (label != blank and (label differs from
      the frame before or the frame starts a read, the read-start flags scattered from read_frames));
      alphabet[labels[mask]] (a boolean-mask compaction, which waits on the host); cumsum(mask) gathered at
      read_frames for the reads' offsets.  It makes neither base_frame nor base_score nor a status.
torch's bases and offsets are compared with d's before any time counts.  The claim under test is d < t by more
than the spread of both over their runs; the tool prints the verdict and changes nothing to make it hold.

    python tools/ctc_timing.py [--reads N] [--frames-per-read n] [--runs R] [--steps K] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1 << 27  # frames whose scores are made at a time


def make_scores(torch, frames, blank, seed):
    """Fill frames [F, 5] float16 chunk by chunk; a run's label is a hash of its number."""
    F, C_ = frames.shape
    gen = torch.Generator(device=frames.device)
    gen.manual_seed(seed)
    for k, lo in enumerate(range(0, F, CHUNK)):
        n = min(CHUNK, F - lo)
        run = torch.cumsum(torch.rand(n, device=frames.device, generator=gen) < 0.4, 0) + k * 7919
        label = ((run * 2654435761) >> 11) % C_
        part = frames[lo:lo + n]
        part.copy_(torch.rand((n, C_), device=frames.device, generator=gen) - 1.0)
        part.scatter_add_(1, label[:, None], torch.full((n, 1), 2.0, dtype=frames.dtype, device=frames.device))
        del run, label


def main(argv=None):
    import torch

    import bench
    from rawnanoporesignalcompression_amd import PGNanoCodec

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--frames-per-read", type=int, default=bdef.samples // 5)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    C_, blank, alphabet = 5, 0, "NACGT"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        """One figure per run: the mean over `steps` steps, after `warmup` steps."""
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
        return f"{name} {sum(runs) / len(runs):9.2f} ms (runs " + ", ".join(f"{v:.2f}" for v in runs) + ")"

    say(f"ctc_timing: {torch.cuda.get_device_name(0)}, {args.reads} reads x {args.frames_per_read} frames, C {C_} float16, "
        f"blank {blank}, {args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    copy_gbs = bench.stream_copy_gbs(torch)
    say(f"stream_copy_gbs {copy_gbs:.1f} (read + write bytes of a device-to-device copy)")

    codec = PGNanoCodec(0)
    alpha = torch.tensor(list(alphabet.encode()), dtype=torch.uint8, device=dev)

    def torch_route(frames, rf):
        labels = frames.argmax(1)
        emit = torch.ones(labels.shape, dtype=torch.bool, device=dev)
        torch.ne(labels[1:], labels[:-1], out=emit[1:])
        emit[rf[:-1]] = True                       # every read here has frames, so each start is a frame
        emit &= labels != blank
        seq = alpha[labels[emit]]
        run = torch.cumsum(emit, 0)
        bases = torch.where(rf > 0, run[(rf - 1).clamp(min=0)], torch.zeros_like(rf))
        return seq, bases

    R = args.reads
    while True:
        F = R * args.frames_per_read
        try:
            frames = torch.empty((F, C_), dtype=torch.float16, device=dev)
            make_scores(torch, frames, blank, args.seed)
            rf = torch.arange(R + 1, dtype=torch.int64, device=dev) * args.frames_per_read
            dec = codec.ctc_decode(frames, rf, codes=True, stream=codec.stream)
            tseq, tbases = torch_route(frames, rf)
            torch.cuda.synchronize()
            break
        except RuntimeError as e:  # out of memory, or a torch op that refuses this many elements
            frames = rf = dec = tseq = tbases = None
            torch.cuda.empty_cache()
            if R <= 1:
                raise
            why = "do not fit the device beside the torch route's intermediates" if isinstance(e, torch.cuda.OutOfMemoryError) \
                else f"make the torch route fail ({str(e).splitlines()[0][:120]})"
            say(f"{R} reads {why}: halving for every quantity")
            R //= 2
    total = int(dec.read_bases[-1].item())
    say(f"{R} reads, {F} frames ({F * C_ * 2 / 1e9:.1f} GB of scores), {total} bases ({100.0 * total / F:.1f} % of the frames emit)")
    same = bool(torch.equal(tbases, dec.read_bases)) and tseq.numel() == total and bool(torch.equal(tseq, dec.seq[:total]))
    say(f"torch's bases and read offsets equal ctc_decode's: {same}; statuses all 0: {bool((dec.status == 0).all().item())}")
    col = codec.collapse_codes(dec.codes, rf, alphabet, stream=codec.stream)
    say("collapse_codes on ctc_decode's codes gives its seq, base_frame and read_bases: "
        f"{bool(torch.equal(col.seq[:total], dec.seq[:total]) and torch.equal(col.base_frame[:total], dec.base_frame[:total]) and torch.equal(col.read_bases, dec.read_bases))}")
    codes = dec.codes
    del tseq, tbases, col, dec
    torch.cuda.empty_cache()

    td = timed(lambda: codec.ctc_decode(frames, rf, stream=codec.stream))
    md = sum(td) / len(td)
    # read: scores, read_frames, the codes again; written: codes, and per base seq + base_frame + base_score
    # (9 bytes) plus the 2-byte winning score gathered for it
    nbytes = F * C_ * 2 + 2 * F + total * (9 + 2) + (R + 1) * 16 + R * 4
    say(fmt("d ctc_decode, all outputs", td) +
        f": {nbytes / 1e9:.1f} GB read + written = {nbytes / (md * 1e-3) / 1e9:.0f} GB/s (stream_copy_gbs {copy_gbs:.0f})")
    tn = timed(lambda: codec.ctc_decode(frames, rf, base_frame=False, base_score=False, stream=codec.stream))
    say(fmt("d' ctc_decode, seq and read_bases only (what the torch route makes)", tn))
    tc = timed(lambda: codec.collapse_codes(codes, rf, alphabet, stream=codec.stream))
    mc = sum(tc) / len(tc)
    cbytes = 2 * F + total * 5 + (R + 1) * 16 + R * 4
    say(fmt("c collapse_codes alone", tc) + f": {cbytes / 1e9:.1f} GB read + written = {cbytes / (mc * 1e-3) / 1e9:.0f} GB/s")
    if same:
        tt = timed(lambda: torch_route(frames, rf))
        mt = sum(tt) / len(tt)
        margin = (max(td) - min(td)) + (max(tt) - min(tt))
        say(fmt("t torch route (argmax, emit mask, labels[mask], cumsum at read_frames)", tt))
        say(f"d < t by more than the spread of both: {mt - md > margin} (d {md:.2f} ms, t {mt:.2f} ms; spreads {margin:.2f} ms)")
    else:
        say("the torch route does not give ctc_decode's bases: no verdict")
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
