#!/usr/bin/env python3
"""CRF posteriors (quality.crf_posteriors over pgn_crf_posterior_rows_device) against the torch route, at
tools/crf_timing.py's shape: float16 scores, T = 2,000 frames per row, state lengths 3, 4 and 5 with 5 transitions
(C = 320, 1,280, 5,120), N = 8,192 / 2,048 / 512 rows (about 10 GB of scores each), one process, HIP events on the
caller's stream.  If the scores and the torch route's forward vectors do not fit the device together, N is halved for
every quantity alike and the log says which ran.  The scores are made on the device: uniform in [-4, 4), float16.

Quantities per state length (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  v   crf_viterbi, the call that reads the same rows once
  p   crf_posteriors at the default scratch cap (1 GiB: rows in groups of floor(cap / (4 * S * T)), the log says how many)
  P   crf_posteriors with the cap raised to hold every row's forward vectors: one launch
  t   the torch route: a loop over t of torch.logsumexp over the gathered [N, S, 5] candidates forward (the vectors
      kept, renormalised by their first element as the device does) and backward, the marginals by a logsumexp over
      the states of each newest base and a softmax over the four
The bytes a posterior call moves are counted from the shapes: the scores twice, the forward vectors written and read
back, the probabilities written; over the call's time that is the rate beside stream_copy_gbs (read + write bytes of a
device-to-device copy) measured in this process.  torch's probabilities are compared with the device's before any time
counts.  The claim under test is P < t and p < t by more than the spread of both over their runs; the tool prints the
verdict and changes nothing to make it hold.

    python tools/crf_post_timing.py [--state-lens 3,4,5] [--frames T] [--gb 10] [--runs R] [--steps K] [--no-torch] [--out FILE]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import torch

    import bench
    from rawnanoporesignalcompression_amd import PGNanoCodec, quality

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--state-lens", default="3,4,5")
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--gb", type=float, default=10.0, help="bytes of scores per state length")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--no-torch", action="store_true", help="skip the torch route")
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    T = args.frames
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

    say(f"crf_post_timing: {torch.cuda.get_device_name(0)}, T {T} frames per row, float16, 5 transitions, about {args.gb:g} GB "
        f"of scores per state length, {args.runs} runs x {args.steps} steps, warmup {args.warmup}"
        + (f", library {os.environ['PGN_LIB']}" if os.environ.get("PGN_LIB") else ""))
    copy_gbs = bench.stream_copy_gbs(torch)
    say(f"stream_copy_gbs {copy_gbs:.1f} (read + write bytes of a device-to-device copy)")
    codec = PGNanoCodec(0)
    default_cap = 1 << 30

    def torch_route(x, k):
        N, S = x.shape[0], 4 ** k
        s_idx = torch.arange(S, device=dev)
        pred = torch.stack([(b * S + s_idx) >> 2 for b in range(4)], 1)                    # p(s, b) as [S, 4]
        succ = torch.stack([((s_idx << 2) | n) & (S - 1) for n in range(4)], 1)            # c(u, n) as [S, 4]
        top = (s_idx >> (2 * k - 2))[:, None].expand(S, 4)
        fwd = torch.empty((T, N, S), dtype=torch.float32, device=dev)
        a = torch.zeros((N, S), dtype=torch.float32, device=dev)
        for t in range(T):
            xt = x[:, t].float().view(N, S, 5)
            a = a - a[:, :1]
            a = torch.logsumexp(torch.cat([a.unsqueeze(2), a[:, pred]], 2) + xt, 2)
            fwd[t] = a
        post = torch.empty((N, T, 4), dtype=torch.float32, device=dev)
        b = torch.zeros((N, S), dtype=torch.float32, device=dev)
        for t in range(T - 1, -1, -1):
            xt = x[:, t].float().view(N, S, 5)
            post[:, t] = torch.softmax(torch.logsumexp((fwd[t] + b).view(N, S // 4, 4), 1), 1)
            b = b - b[:, :1]
            moves = xt[:, succ, 1 + top]                                                    # move(t, c(u, n), top(u))
            b = torch.logsumexp(torch.cat([(b + xt[:, :, 0]).unsqueeze(2), b[:, succ] + moves], 2), 2)
        return post

    for k in [int(v) for v in args.state_lens.split(",")]:
        S = 4 ** k
        C_ = 5 * S
        N = 1 << max(0, round(math.log2(args.gb * 1e9 / (T * C_ * 2))))  # the power of two nearest to --gb of scores
        while True:
            try:
                gen = torch.Generator(device=dev)
                gen.manual_seed(args.seed + k)
                x = torch.empty((N, T, C_), dtype=torch.float16, device=dev)
                for lo in range(0, N, max(1, N // 16)):
                    part = x[lo:lo + max(1, N // 16)]
                    part.copy_(torch.rand(part.shape, device=dev, generator=gen) * 8 - 4)
                codec.set_crf_scratch(0)
                out = torch.empty((N, T, 4), dtype=torch.float32, device=dev)
                got = quality.crf_posteriors(codec, x, k, out=out, stream=codec.stream)
                want = None if args.no_torch else torch_route(x, k)
                torch.cuda.synchronize()
                break
            except RuntimeError as e:
                x = out = got = want = None
                torch.cuda.empty_cache()
                if N <= 1:
                    raise
                say(f"k {k}: {N} rows do not run ({str(e).splitlines()[0][:100]}): halving for every quantity")
                N //= 2
        nbytes = N * T * C_ * 2
        row_bytes = 4 * S * T
        group = default_cap // row_bytes
        moved = 2 * nbytes + 2 * N * row_bytes + N * T * 16
        say(f"k {k}: S {S}, C {C_}, N {N} rows, {nbytes / 1e9:.2f} GB of scores, forward vectors {row_bytes / 1e6:.2f} MB per "
            f"row and {N * row_bytes / 1e9:.2f} GB in all; the default cap holds {group} rows: {-(-N // group)} launches")
        say(f"  a call moves {moved / 1e9:.2f} GB: the scores twice, the forward vectors out and back, the probabilities")
        if want is not None:
            diff = float((want - got).abs().max().item())
            say(f"  torch's probabilities against crf_posteriors': max |difference| {diff:.3e}")
        del want
        torch.cuda.empty_cache()
        codec.set_crf_scratch(N * row_bytes)
        raised = quality.crf_posteriors(codec, x, k, stream=codec.stream)
        torch.cuda.synchronize()
        say(f"  the raised cap gives the default cap's bits: {bool(torch.equal(raised, got))}")
        del raised
        codes = torch.empty((N, T), dtype=torch.uint8, device=dev)
        tv = timed(lambda: codec.crf_viterbi(x, k, codes=codes, stream=codec.stream))
        mv = sum(tv) / len(tv)
        say("  " + fmt("v crf_viterbi", tv) + f": {nbytes / (mv * 1e-3) / 1e9:.0f} GB/s of scores")
        tP = timed(lambda: quality.crf_posteriors(codec, x, k, out=out, stream=codec.stream))
        mP = sum(tP) / len(tP)
        say("  " + fmt("P crf_posteriors, cap raised to hold every row", tP) + f": {moved / (mP * 1e-3) / 1e9:.0f} GB/s moved "
            f"(stream_copy_gbs {copy_gbs:.0f}), {mP / mv:.2f} x v")
        codec.set_crf_scratch(0)
        tp = timed(lambda: quality.crf_posteriors(codec, x, k, out=out, stream=codec.stream))
        mp = sum(tp) / len(tp)
        say("  " + fmt("p crf_posteriors, default cap", tp) + f": {moved / (mp * 1e-3) / 1e9:.0f} GB/s moved, {mp / mv:.2f} x v")
        if not args.no_torch:
            tt = timed(lambda: torch_route(x, k))
            mt = sum(tt) / len(tt)
            for name, runs, mean in (("P", tP, mP), ("p", tp, mp)):
                margin = (max(runs) - min(runs)) + (max(tt) - min(tt))
                say(f"  {name} < t by more than the spread of both: {mt - mean > margin} ({name} {mean:.3f} ms, t {mt:.2f} ms; "
                    f"spreads {margin:.3f} ms)")
            say("  " + fmt("t torch route (loops over t of logsumexp over [N, S, 5], both directions)", tt))
        del x, out, got, codes
        torch.cuda.empty_cache()
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
