#!/usr/bin/env python3
"""Model output back to reads: stitch_plan and stitch against torch's best route, at the shape derived from
the bench's (100,000 reads x 100,000 samples, usual head trims, segments of 10,000 with an overlap of 500, a
model of stride 5, frames of 16 bytes), one process, HIP events on the caller's stream.

The segment table is built on the host from the segment rule for reads whose trims are drawn uniformly from
[0, 3,400] (the mean the usual trim has on the bench's reads); the "model output" is random int32 bits,
[segments, T, frame_bytes / 4].  If rows, output and the torch route's index and output do not fit the
device together, the frame is halved until they do, and the log says which size ran.

Quantities (each run `--runs` times over `--steps` steps; a run's figure is the mean of its steps):
  p   stitch_plan alone
  g   stitch of the whole table in one call into a preallocated output; its bytes read and written over that
      time, beside stream_copy_gbs measured in this process
  t   the route without this call: the int64 source index of every kept frame, built beforehand (from the
      numpy rule on the host, expanded on the device; not timed), then
      torch.index_select(rows.view(-1, C), 0, index, out=...) into a preallocated output; if that call does not
      return the right frames at this size, torch.take and index_select over the rows seen as a one-dimensional
      tensor of one element per frame
  gT  (with --time-major) stitch of the same frames from a [T, segments, C] copy of the rows
The claim under test is g < t by more than the spread of both over their runs; the tool prints the verdict and
changes nothing to make it hold.  The two outputs must have the same bits; both, and the index, are also checked
at `--probe` random frames against the numpy rule worked out on the host, and where the outputs differ the tool
says how many frames do and which of the two is right at the first.

    python tools/stitch_timing.py [--reads N] [--samples n] [--length L] [--overlap V] [--frame-samples s]
                                  [--frame-bytes B] [--time-major] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_tables(R, n, L, V, max_trim, seed):
    """pgn_read_segments and pgn_segment records of R reads of n samples with random trims, as the segment
    call leaves them."""
    from rawnanoporesignalcompression_amd import ReadSegments, SegmentTable

    rng = np.random.default_rng(seed)
    S = L - V
    trim = rng.integers(0, max_trim + 1, R).astype(np.int64)
    m = n - trim
    k = np.where(m > L, (np.maximum(m - L, 0) + S - 1) // S + 1, (m > 0).astype(np.int64))
    first = np.cumsum(k) - k
    total = int(k.sum())
    reads = np.zeros(R, ReadSegments.DTYPE)
    reads["first_segment"], reads["nsegments"], reads["trim"] = first, k, trim
    read = np.repeat(np.arange(R), k)
    j = np.arange(total) - np.repeat(first, k)
    segs = np.zeros(total, SegmentTable.DTYPE)
    segs["read"] = read
    segs["start"] = trim[read] + np.minimum(j * S, np.maximum(m[read] - L, 0))
    segs["valid"] = np.minimum(m[read], L)
    return reads, segs, m, k


def main(argv=None):
    import torch

    import bench
    from rawnanoporesignalcompression_amd import (PGNanoCodec, ReadSegments, SegmentedReads, SegmentTable,
                                                  stitch_plan_signal)

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reads", type=int, default=100_000)
    p.add_argument("--samples", type=int, default=bdef.samples, help="samples per read")
    p.add_argument("--length", type=int, default=10_000)
    p.add_argument("--overlap", type=int, default=500)
    p.add_argument("--frame-samples", type=int, default=5)
    p.add_argument("--frame-bytes", type=int, default=16, help="a multiple of 4")
    p.add_argument("--max-trim", type=int, default=3400)
    p.add_argument("--probe", type=int, default=100_000, help="frames checked against the numpy rule on the host")
    p.add_argument("--time-major", action="store_true", help="also time a [T, segments, C] copy of the rows")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    R, n, L, V, s = args.reads, args.samples, args.length, args.overlap, args.frame_samples
    T = L // s
    dev = torch.device("cuda", 0)
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

    say(f"stitch_timing: {torch.cuda.get_device_name(0)}, {R} reads x {n} samples, trims up to {args.max_trim}, L {L}, "
        f"V {V}, s {s} (T {T}), {args.runs} runs x {args.steps} steps, warmup {args.warmup}")
    copy_gbs = bench.stream_copy_gbs(torch)
    say(f"stream_copy_gbs {copy_gbs:.1f} (read + write bytes of a device-to-device copy)")

    reads, segs, m, k = host_tables(R, n, L, V, args.max_trim, args.seed)
    total = len(segs)
    # the numpy rule per read (reads of one length share it), then per segment: source frame and count
    rule = {}
    for mm in np.unique(m):
        rule[int(mm)] = stitch_plan_signal(int(mm), L, V, s)
    fc = np.concatenate([rule[int(mm)] for mm in m]) if total else np.zeros((0, 2), np.int64)
    frames = int(fc[:, 1].sum())
    say(f"{total} segments, {frames} frames kept of {total * T} ({100.0 * frames / max(total * T, 1):.2f} %)")

    codec = PGNanoCodec(0)
    raw = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1)).to(dev)
    seg = SegmentedReads(None, SegmentTable(raw(segs)), ReadSegments(raw(reads)), None,
                         torch.tensor(total, dtype=torch.int64, device=dev))
    plan = codec.stitch_plan(seg, L, V, s, stream=codec.stream)
    got = plan.segments.numpy()
    assert np.array_equal(got["first"], fc[:, 0]) and np.array_equal(got["count"], fc[:, 1])
    assert int(plan.read_frames[-1].item()) == frames
    tp = timed(lambda: codec.stitch_plan(seg, L, V, s, stream=codec.stream))
    say(fmt("p stitch_plan alone", tp))

    fb = args.frame_bytes
    while True:
        C = fb // 4
        try:
            rows = torch.empty((total, T, C), dtype=torch.int32, device=dev)
            rows.random_()
            out = torch.empty((frames, C), dtype=torch.int32, device=dev)
            tout = torch.empty((frames, C), dtype=torch.int32, device=dev)
            src = torch.from_numpy(np.arange(total, dtype=np.int64) * T + fc[:, 0]).to(dev)
            cnt = torch.from_numpy(fc[:, 1].copy()).to(dev)
            index = torch.repeat_interleave(src - (torch.cumsum(cnt, 0) - cnt), cnt)
            index += torch.arange(frames, dtype=torch.int64, device=dev)
            del src, cnt
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            rows = out = tout = index = None
            torch.cuda.empty_cache()
            if fb <= 4:
                raise
            say(f"frames of {fb} bytes do not fit the device beside the torch route's index and output: halving")
            fb //= 2
    say(f"frames of {fb} bytes: rows {rows.numel() * 4 / 1e9:.1f} GB, output {out.numel() * 4 / 1e9:.1f} GB, "
        f"torch index {index.numel() * 8 / 1e9:.1f} GB")

    tg = timed(lambda: codec.stitch(plan, rows, out=out, stream=codec.stream))
    nbytes = 2 * frames * fb
    mg = sum(tg) / len(tg)
    say(fmt("g stitch, the whole table in one call", tg) +
        f": {nbytes / 1e9:.1f} GB read + written = {nbytes / (mg * 1e-3) / 1e9:.0f} GB/s (stream_copy_gbs {copy_gbs:.0f})")
    flat = rows.view(-1, C)
    # the frames at which both outputs and the index are checked against the numpy rule, worked out on the host
    probe = np.sort(np.random.default_rng(args.seed).integers(0, max(frames, 1), args.probe))
    starts = np.cumsum(fc[:, 1]) - fc[:, 1]
    row = np.searchsorted(starts, probe, side="right") - 1
    frame = fc[row, 0] + probe - starts[row]
    d_probe = torch.from_numpy(probe).to(dev)
    want = torch.stack([rows[int(r)][int(f)] for r, f in zip(row[:256], frame[:256])])  # by selects, no gather kernel
    if torch.equal(rows[torch.from_numpy(row[:256]).to(dev), torch.from_numpy(frame[:256]).to(dev)], want):
        want = rows[torch.from_numpy(row).to(dev), torch.from_numpy(frame).to(dev)]
    else:
        say("torch's indexing of the rows by (row, frame) pairs is wrong at this size: 256 frames are checked, by selects")
        probe, row, frame, d_probe = probe[:256], row[:256], frame[:256], d_probe[:256]
    index_ok = int((index[d_probe] == torch.from_numpy(row * T + frame).to(dev)).sum().item())
    say(f"{len(probe)} random frames against the numpy rule on the host: g {int((out[d_probe] == want).all(1).sum().item())} "
        f"right, index entries {index_ok} right")

    # The torch route.  index_select over the whole index is the route; at this size it has been seen to return
    # wrong frames (a stretch of the output a power of two of bytes long, from 2 GiB of output on; advanced
    # indexing with the same index returns the same, and in pieces of 2^26 or 2^28 frames the call is refused with
    # an invalid launch configuration), so two more forms are timed when it does, both over the rows seen as a
    # one-dimensional tensor of one element per frame: torch.take and index_select.  A form counts only if it
    # gives g's bits; the verdict is against the fastest that does.
    wide = {16: torch.complex128, 8: torch.int64, 4: torch.int32}[fb]
    flat1, tout1 = rows.view(wide).view(-1), tout.view(wide).view(-1)

    def one_call():
        torch.index_select(flat, 0, index, out=tout)

    def take_wide():
        torch.take(flat1, index, out=tout1)

    def select_wide():
        torch.index_select(flat1, 0, index, out=tout1)

    right = []
    for name, route, upto, scale in (("index_select, one call", one_call, frames, 1),
                                     (f"take, frames as {wide} elements", take_wide, frames, 1),
                                     (f"index_select, frames as {wide} elements", select_wide, frames, 1)):
        if right and right[0][0] == "index_select, one call":
            break
        tout.zero_()
        try:
            runs = timed(route)
            res = tout
            same = torch.equal(out[:upto], res[:upto])
            inside = torch.from_numpy(probe < upto).to(dev)
            hit = int((res[d_probe[inside]] == want[inside]).all(1).sum().item())
        except RuntimeError as e:
            say(f"t torch {name}: {str(e).splitlines()[0]}")
            continue
        say(fmt(f"t torch {name}", runs) + f"; same bits as g: {same}; {hit} of {int(inside.sum())} random frames right")
        if same:
            right.append((name, [v * scale for v in runs], scale))
            continue
        differ, first = 0, None
        for lo in range(0, upto, 1 << 26):
            hi = min(lo + (1 << 26), upto)
            bad = (out[lo:hi] != res[lo:hi]).any(1)
            nbad = int(bad.sum().item())
            if nbad and first is None:
                first = lo + int(bad.nonzero()[0].item())
            differ += nbad
        r1 = int(np.searchsorted(starts, first, side="right") - 1)
        f1 = int(fc[r1, 0] + first - starts[r1])
        one = rows[r1][f1]
        say(f"   g and t differ in {differ} frames of {upto}, first at frame {first} (row {r1} frame {f1}): g right "
            f"{bool((out[first] == one).all().item())}, t right {bool((res[first] == one).all().item())}, "
            f"index {int(index[first].item())} want {r1 * T + f1}")
        del res
    if not right:
        say("no form of the torch route gave g's bits: no verdict")
    else:
        name, tt, scale = min(right, key=lambda r: sum(r[1]))
        mt = sum(tt) / len(tt)
        margin = (max(tg) - min(tg)) + (max(tt) - min(tt))
        say(f"g < t by more than the spread of both: {mt - mg > margin} (g {mg:.2f} ms, t {mt:.2f} ms: {name}"
            + (f", scaled by {scale}" if scale > 1 else "") + f"; spreads {margin:.2f} ms)")
    res = None
    del flat1, tout1
    del tout, index, flat
    torch.cuda.empty_cache()
    if args.time_major:
        try:
            rows_t = rows.transpose(0, 1).contiguous()
            keep = out.clone()
            out.zero_()
            tgt = timed(lambda: codec.stitch(plan, rows_t, out=out, time_major=True, stream=codec.stream))
            mgt = sum(tgt) / len(tgt)
            say(fmt("gT stitch from [T, segments, C] rows", tgt) +
                f": {nbytes / (mgt * 1e-3) / 1e9:.0f} GB/s; same bits as g: {torch.equal(out, keep)}")
        except torch.cuda.OutOfMemoryError:
            say("gT: no room on the device for the [T, segments, C] copy")
    codec.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
