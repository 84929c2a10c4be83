#!/usr/bin/env python3
"""CRF model rows to per-frame codes: crf_viterbi against the torch route, at the shape derived from the bench's
(rows of L = 10,000 samples at a model stride of 5: T = 2,000 frames, float16 scores), for state lengths 3, 4 and
5 with 5 transitions (C = 320, 1,280, 5,120), one process, HIP events on the caller's stream.

N is chosen per state length so that the scores take about 10 GB (8,192, 2,048 and 512 rows); if the scores and
the torch route's backpointers do not fit the device together, N is halved for every quantity alike and the log
says which ran.  The scores are made on the device: uniform in [-4, 4), rounded to float16.

Quantities per state length (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  f   crf_viterbi as shipped (the traceback in the row's own workgroup): codes and row_score; the bytes of scores
      read over that time, beside stream_copy_gbs measured in this process
  n   the forward pass alone (a context made with PGN_CRF_TRACEBACK=none): f's forward share is n / f
  s   the other placement of the traceback (PGN_CRF_TRACEBACK=split: a second kernel, a lane per row)
  t   the torch route: a host loop over t of torch.max over the gathered [N, S, 5] candidates (stay first, then
      b = 0..3, the rule's order), then a traceback by gather; the same codes and row scores
torch's codes and scores are compared with f's before any time counts, and the log says how many differ (torch.max
does not promise the lowest index on a tie).  The claim under test is f < t by more than the spread of both over
their runs; the tool prints the verdict and changes nothing to make it hold.

    python tools/crf_timing.py [--state-lens 3,4,5] [--frames T] [--gb 10] [--runs R] [--steps K] [--no-torch] [--out FILE]
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
    from rawnanoporesignalcompression_amd import PGNanoCodec

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--state-lens", default="3,4,5")
    p.add_argument("--frames", type=int, default=2000)
    p.add_argument("--gb", type=float, default=10.0, help="bytes of scores per state length")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--no-torch", action="store_true", help="skip the torch route (variant builds: f, n and s only)")
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

    def context(mode):
        if mode:
            os.environ["PGN_CRF_TRACEBACK"] = mode
        try:
            return PGNanoCodec(0)
        finally:
            os.environ.pop("PGN_CRF_TRACEBACK", None)

    say(f"crf_timing: {torch.cuda.get_device_name(0)}, T {T} frames per row, float16, 5 transitions, about {args.gb:g} GB of "
        f"scores per state length, {args.runs} runs x {args.steps} steps, warmup {args.warmup}"
        + (f", library {os.environ['PGN_LIB']}" if os.environ.get("PGN_LIB") else ""))
    copy_gbs = bench.stream_copy_gbs(torch)
    say(f"stream_copy_gbs {copy_gbs:.1f} (read + write bytes of a device-to-device copy)")
    fused, forward_only, split = context(None), context("none"), context("split")

    def torch_route(x, k):
        N, S = x.shape[0], 4 ** k
        a = torch.zeros((N, S), dtype=torch.float32, device=dev)
        bp = torch.empty((T, N, S), dtype=torch.uint8, device=dev)
        s_idx = torch.arange(S, device=dev)
        pred = torch.stack([(b * S + s_idx) >> 2 for b in range(4)], 1)   # [S, 4]
        for t in range(T):
            xt = x[:, t].float().view(N, S, 5)
            cand = torch.cat([a.unsqueeze(2), a[:, pred]], 2) + xt
            a, j = cand.max(2)
            bp[t] = j
        m, s = a.max(1)
        codes = torch.empty((N, T), dtype=torch.uint8, device=dev)
        for t in range(T - 1, -1, -1):
            j = bp[t].gather(1, s[:, None]).squeeze(1).long()
            codes[:, t] = ((s & 3) | ((j > 0) * 128)).to(torch.uint8)
            s = torch.where(j > 0, ((j - 1) * S + s) >> 2, s)
        return codes, m

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
                got = fused.crf_viterbi(x, k, stream=fused.stream)
                want = None if args.no_torch else torch_route(x, k)
                torch.cuda.synchronize()
                break
            except RuntimeError as e:
                x = got = want = None
                torch.cuda.empty_cache()
                if N <= 1:
                    raise
                say(f"k {k}: {N} rows do not run ({str(e).splitlines()[0][:100]}): halving for every quantity")
                N //= 2
        nbytes = N * T * C_ * 2
        say(f"k {k}: S {S}, C {C_}, N {N} rows, {nbytes / 1e9:.2f} GB of scores, scratch "
            f"{N * (4 * S * ((T + 7) // 8) + 16) / 1e6:.0f} MB")
        other = split.crf_viterbi(x, k, stream=split.stream)
        torch.cuda.synchronize()
        say(f"  the split traceback gives the same codes and scores: "
            f"{bool(torch.equal(other.codes, got.codes) and torch.equal(other.row_score.view(torch.int32), got.row_score.view(torch.int32)))}")
        same = None
        if want is not None:
            dc = int((want[0] != got.codes).sum().item())
            ds = int((want[1].view(torch.int32) != got.row_score.view(torch.int32)).sum().item())
            rows_c = int((want[0] != got.codes).any(1).sum().item())
            same = dc == 0 and ds == 0
            say(f"  torch's codes and row scores equal crf_viterbi's: {same} ({dc} of {N * T} code bytes in {rows_c} rows and "
                f"{ds} of {N} row scores differ)")
        del other, want
        torch.cuda.empty_cache()
        tf = timed(lambda: fused.crf_viterbi(x, k, stream=fused.stream))
        mf = sum(tf) / len(tf)
        say("  " + fmt("f crf_viterbi", tf) + f": {nbytes / 1e9:.2f} GB of scores read = {nbytes / (mf * 1e-3) / 1e9:.0f} GB/s "
            f"(stream_copy_gbs {copy_gbs:.0f} counts read + write)")
        tn = timed(lambda: forward_only.crf_viterbi(x, k, stream=forward_only.stream))
        mn = sum(tn) / len(tn)
        say("  " + fmt("n forward pass alone", tn) + f": forward share {100 * mn / mf:.0f} %, traceback share {100 * (mf - mn) / mf:.0f} % of f")
        ts = timed(lambda: split.crf_viterbi(x, k, stream=split.stream))
        ms_ = sum(ts) / len(ts)
        say("  " + fmt("s traceback as a second kernel, a lane per row", ts) + f": its traceback {ms_ - mn:.3f} ms against {mf - mn:.3f} ms")
        if not args.no_torch:
            tt = timed(lambda: torch_route(x, k))
            mt = sum(tt) / len(tt)
            margin = (max(tf) - min(tf)) + (max(tt) - min(tt))
            say("  " + fmt("t torch route (loop over t of max over [N, S, 5], traceback by gather)", tt))
            say(f"  f < t by more than the spread of both: {mt - mf > margin} (f {mf:.3f} ms, t {mt:.2f} ms; spreads {margin:.3f} ms; "
                f"torch returns the same bits: {same})")
        del x, got
        torch.cuda.empty_cache()
    for c in (fused, forward_only, split):
        c.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
