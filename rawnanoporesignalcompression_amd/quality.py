"""Per-base qualities for the CRF route (include/pgnano_hip.h, "Posteriors and qualities (CRF)"): the posterior
marginals of a model's rows and the phred string made of them, as functions that take the codec.

The package's ``__all__`` and the methods of :class:`~rawnanoporesignalcompression_amd.codec.PGNanoCodec` are a
fixed surface, so the two device calls live here.  They run inside the codec's launch scope and check their
arguments with the helpers the codec's own methods use.  For table rows ``[first, first + N)`` of a segmented
batch::

    scores = model(rows)
    codes = codec.crf_viterbi(scores, state_len).codes
    post = quality.crf_posteriors(codec, scores, state_len)
    codec.stitch(plan, codes, first, out=frame_codes)            # one byte per frame
    codec.stitch(plan, post, first, out=frame_post)              # sixteen bytes per frame
    bases = codec.collapse_codes(frame_codes, plan.read_frames, "ACGT")
    qual = quality.base_qual(codec, bases, frame_codes, frame_post, plan.read_frames)

``bases.seq`` and ``qual`` are then the second and the fourth line of every read's FASTQ record.  The host models
(:func:`crf_posteriors_signal`, :func:`base_qual_signal`, :func:`qual_thresholds`, :func:`qual_params`) are those
of :mod:`~rawnanoporesignalcompression_amd.host`.
"""
from __future__ import annotations

import ctypes as C

from .codec import DecodedReads, PGNanoCodec, _check, _crf_rows, _ptr, _require_device, _require_out
from .host import base_qual_signal, crf_posteriors_signal, qual_params, qual_thresholds

__all__ = ["crf_posteriors", "base_qual", "crf_posteriors_signal", "base_qual_signal", "qual_thresholds", "qual_params"]


def crf_posteriors(codec: PGNanoCodec, rows, state_len, *, transitions=None, stay_score=0.0, time_major: bool = False,
                   out=None, stream: int | None = None):
    """The posterior marginals of a CRF model's rows (pgn_crf_posterior_rows_device): per row
    :func:`crf_posteriors_signal` of its scores, in float32, to four times that model's own float32 error.

    rows, ``state_len``, ``transitions``, ``stay_score`` and ``time_major`` are those of
    :meth:`PGNanoCodec.crf_viterbi`.  out: a float32 ``[N, T, 4]`` tensor to write into, its last two dimensions
    contiguous and its row stride at least ``4 * T`` (default: a new one).  Returns it: ``out[g, t, b]`` is the
    probability that the newest base of row ``g``'s state after frame ``t`` is ``b``.  The scratch is 4 bytes per
    state and frame of a row, under the cap of :meth:`PGNanoCodec.set_crf_scratch`.  No host wait."""
    import torch

    prm, N, T, nd, td = _crf_rows(rows, state_len, transitions, stay_score, time_major, codec.device)
    item = rows.element_size()
    with codec._launch(stream) as ls:
        if out is None:
            out = torch.empty((N, T, 4), dtype=torch.float32, device=rows.device)
        else:
            _require_out(out, "out", codec.device, torch.float32)
            if (tuple(out.shape) != (N, T, 4) or out.stride(2) != 1 or (T > 1 and out.stride(1) != 4)
                    or (N > 1 and out.stride(0) < 4 * T)):
                raise ValueError(f"out must be a float32 [{N}, {T}, 4] tensor, rows contiguous and at least 4 * T apart")
        if N:
            _check(codec._lib.pgn_crf_posterior_rows_device(
                codec._h, C.byref(prm), N, T, _ptr(rows), int(rows.stride(nd)) * item, int(rows.stride(td)) * item,
                _ptr(out), max(int(out.stride(0)), 4 * T) if N > 1 else 4 * T, ls.cuda_stream))
    return out


def base_qual(codec: PGNanoCodec, decoded: DecodedReads, codes, post, read_frames, thresholds=None, *, q_min: int = 1,
              frame_base: int = 0, out=None, stream: int | None = None):
    """One phred character per base (pgn_base_qual_device): per read :func:`base_qual_signal` of its stitched
    codes and probabilities, bit for bit.

    decoded: what :meth:`PGNanoCodec.collapse_codes` returned for ``codes`` and ``read_frames`` with the same
    ``frame_base`` (made with ``base_frame=True``).  codes: uint8, contiguous, ``codes[i - frame_base]`` for frame
    ``i``; post: float32 ``[frames, 4]`` contiguous, the stitched output of :func:`crf_posteriors`.  thresholds:
    non-increasing uint32 values (default :func:`qual_thresholds` from ``q_min`` to 50); a base's quality is
    ``q_min`` plus the number of thresholds its mean error does not exceed.  out: a uint8 tensor of
    ``decoded.seq``'s size (default: a new one).  Returns it: read ``r``'s string is ``out[read_bases[r]:
    read_bases[r + 1]]``; the bytes of reads with a status, outside the window or cut by the capacity are not
    written.  No host wait."""
    import torch

    _require_device(codes, "codes", codec.device)
    if codes.dtype != torch.uint8 or codes.dim() != 1 or not codes.is_contiguous():
        raise ValueError("codes must be a contiguous one-dimensional uint8 tensor")
    F = int(codes.numel())
    _require_device(post, "post", codec.device)
    if post.dtype != torch.float32 or tuple(post.shape) != (F, 4) or not post.is_contiguous():
        raise ValueError(f"post must be a contiguous float32 [{F}, 4] tensor, a frame per code byte")
    _require_device(read_frames, "read_frames", codec.device)
    if read_frames.dtype != torch.int64 or read_frames.dim() != 1 or read_frames.numel() < 1 or not read_frames.is_contiguous():
        raise ValueError("read_frames must be a contiguous int64 tensor of reads + 1 offsets")
    n = int(read_frames.numel()) - 1
    if decoded.base_frame is None:
        raise ValueError("decoded must carry base_frame (collapse_codes(..., base_frame=True))")
    for name, t, size in (("read_bases", decoded.read_bases, n + 1), ("status", decoded.status, n)):
        _require_device(t, f"decoded.{name}", codec.device)
        if int(t.numel()) != size or not t.is_contiguous():
            raise ValueError(f"decoded.{name} must hold {size} entries, as for read_frames")
    capacity = int(decoded.seq.numel())
    _require_device(decoded.base_frame, "decoded.base_frame", codec.device)
    if int(decoded.base_frame.numel()) < capacity or not decoded.base_frame.is_contiguous():
        raise ValueError("decoded.base_frame must hold an entry per base of decoded.seq")
    prm = qual_params(thresholds, q_min)
    frame_base = int(frame_base)
    if not 0 <= frame_base < 1 << 62:
        raise ValueError("frame_base must lie in [0, 2^62)")
    with codec._launch(stream) as ls:
        if out is None:
            out = torch.empty(capacity, dtype=torch.uint8, device=codes.device)
        else:
            _require_out(out, "out", codec.device, torch.uint8)
            if out.dim() != 1 or int(out.numel()) != capacity or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous uint8 tensor of {capacity} bytes")
        _check(codec._lib.pgn_base_qual_device(
            codec._h, C.byref(prm), n, _ptr(read_frames), _ptr(codes) if F else 0, _ptr(post) if F else 0, frame_base, F,
            _ptr(decoded.read_bases), _ptr(decoded.base_frame) if capacity else 0, _ptr(decoded.status),
            _ptr(out) if capacity else 0, capacity, ls.cuda_stream))
    return out
