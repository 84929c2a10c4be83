#!/usr/bin/env python3
"""POD5 file -> calibrated reads in HBM: what the loader costs, in one process, timed with HIP events.

A signal-only POD5 file (pgnano.signal, C5) of synthetic reads is written from synth_reads +
compress_batch + write_pod5, opened natively, and loaded through pgn_pod5_load_row_lists_device as
float16 pA (reads of --rows-per-read rows, the test's own row lists and calibration).

  (a) device time of the per-read calibrated decode (expand kernel, decode, status kernel:
      decompress_reads_pa) against decompress_batch_pa on the same chunks, both on blobs already
      resident, HIP events on the caller's stream, three runs of --steps each.  The difference is the
      two small kernels and should sit inside the run-to-run spread.
  (b) end to end: host gather from the file image into pinned staging, one upload, the decode; wall
      clock around load_reads + a device synchronise, best of --steps after a warm-up, in samples/s,
      beside bench.py's pod5_batch_host decode figure measured in this same process (that path decodes
      rows from host memory and downloads int16; the loader downloads nothing).  A ratio, no verdict.

    python tools/pod5_load_timing.py [--rows N] [--samples L] [--out profiles/pod5_load_timing.log]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch

    import bench
    from rawnanoporesignalcompression_amd import PGNanoCodec
    from rawnanoporesignalcompression_amd.pod5_file import Pod5File, SignalTable, write_pod5

    bdef = bench.parse([])
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000, help="signal rows (chunks) of the file")
    p.add_argument("--samples", type=int, default=bdef.samples, help="samples per row")
    p.add_argument("--rows-per-read", type=int, default=4)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--seed", type=int, default=bdef.seed)
    p.add_argument("--dir", default=None, help="where the file is written (default: a temporary directory)")
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args(argv)
    N, L, K = args.rows, args.samples, args.rows_per_read
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"pod5_load_timing: {torch.cuda.get_device_name(0)}, {N} rows x {L} samples, {K} rows per read, steps {args.steps}")
    codec = PGNanoCodec(0)
    samples, offs, counts = codec.synth_reads(N, L, seed=args.seed)
    enc = codec.compress_batch(samples, offs, counts, stream=codec.stream)
    torch.cuda.synchronize()
    assert bool((enc.status == 0).all().item())
    del samples
    # ---- the file: the blobs packed back to back, one row each
    sizes = enc.sizes.cpu().numpy().astype(np.uint64)
    boffs = enc.offsets.cpu().numpy().astype(np.int64)
    col = np.zeros(N + 1, np.uint64)
    np.cumsum(sizes, out=col[1:])
    hblobs = enc.blobs.cpu().numpy()
    data = np.empty(int(col[-1]), np.uint8)
    for i in range(N):
        data[int(col[i]):int(col[i + 1])] = hblobs[boffs[i]:boffs[i] + int(sizes[i])]
    del hblobs
    ids = np.random.default_rng(args.seed).integers(0, 256, (N, 16)).astype(np.uint8)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    path = os.path.join(tmp.name, "synthetic.pod5")
    write_pod5(path, SignalTable(ids, np.full(N, L, np.uint32), col, data, "pgnano"), source=None)
    say(f"file: {os.path.getsize(path) / 1e6:.1f} MB for {N * L / 1e6:.0f} M samples ({8 * col[-1] / (N * L):.2f} bits/sample)")
    nreads = -(-N // K)
    first = np.minimum(np.arange(nreads + 1, dtype=np.uint64) * K, N).astype(np.uint64)
    rows = np.arange(N, dtype=np.uint64)
    cal_off = (-243.37 + 0.61 * (np.arange(nreads) % 512)).astype(np.float32)
    cal_scale = (0.17553 * (1 + (np.arange(nreads) % 257) / 257)).astype(np.float32)
    out = torch.empty(N * L, dtype=torch.float16, device=dev)

    def events(fn, steps):
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sum(ms) / len(ms), min(ms), max(ms)

    # ---- (a) resident blobs: per-read call against the per-chunk call
    d_first = torch.from_numpy(first.astype(np.int64)).to(dev)
    d_ro = d_first[:-1] * L
    chunk_read = torch.from_numpy(np.repeat(np.arange(nreads), np.diff(first.astype(np.int64)))).to(dev)
    d_off, d_scale = torch.from_numpy(cal_off).to(dev), torch.from_numpy(cal_scale).to(dev)
    c_off, c_scale = d_off[chunk_read].contiguous(), d_scale[chunk_read].contiguous()
    blob = (enc.blobs, enc.offsets, enc.sizes, counts)

    def per_chunk():
        return codec.decompress_batch_pa(*blob, c_off, c_scale, dtype=torch.float16, out=out, out_offsets=offs,
                                         stream=codec.stream, max_chunk_samples=L)

    def per_read():
        return codec.decompress_reads_pa(*blob, d_first, d_off, d_scale, dtype=torch.float16, out=out,
                                         read_out_offsets=d_ro, stream=codec.stream, max_chunk_samples=L)

    per_chunk()
    want = out.clone()
    out.zero_()
    st = per_read()[2]
    torch.cuda.synchronize()
    assert bool((st == 0).all().item()) and torch.equal(out.view(torch.int16), want.view(torch.int16))
    for run in range(3):
        tc, tr = events(per_chunk, args.steps), events(per_read, args.steps)
        say(f"(a) run {run}: decompress_batch_pa {tc[0]:.3f} ms (min {tc[1]:.3f}, max {tc[2]:.3f}); "
            f"decompress_reads_pa {tr[0]:.3f} ms (min {tr[1]:.3f}, max {tr[2]:.3f}); difference {tr[0] - tc[0]:+.3f} ms")
    # ---- (b) end to end from the open file
    with Pod5File(path) as f:
        def load():
            res = f.load_reads(codec, output="pa", dtype=torch.float16, out=out, row_lists=(first, rows),
                               calibration=(cal_off, cal_scale), stream=codec.stream)
            torch.cuda.synchronize()
            return res

        out.zero_()
        res = load()  # staging at full size; and the same bytes as the resident decode
        assert bool((res.status == 0).all().item()) and torch.equal(out.view(torch.int16), want.view(torch.int16))
        del want
        wall = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            load()
            wall.append(time.perf_counter() - t0)
    best = min(wall)
    say(f"(b) load_reads (gather + upload + decode to float16 pA): best {best * 1e3:.1f} ms of {args.steps} "
        f"(worst {max(wall) * 1e3:.1f} ms) = {N * L / best / 1e6:.0f} Msamples/s")
    del out
    torch.cuda.empty_cache()
    host = bench.pod5_batch_host(torch, codec, L, args.seed)
    say(f"(b) pod5_batch_host decode (rows from host memory, int16 back to host): {host['decode_msamples_s']:.0f} Msamples/s; "
        f"loader / pod5_batch_host = {N * L / best / 1e6 / host['decode_msamples_s']:.2f}")
    codec.close()
    tmp.cleanup()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
