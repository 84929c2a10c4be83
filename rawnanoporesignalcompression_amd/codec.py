"""Host-side mirror of the reference's pgnano plugin surface, over the C ABI.

Reference interface (tomas-gr/RawNanoporeSignalCompression):

* ``pgnano::compress_signal(samples, pool, read_data, is_last_batch) -> Result<Buffer>``
  (pod5/c++/pod5_format/pgnano/pgnano.h:19-23, pgnano.cpp:59-96): allocates
  ``compressed_signal_max_size`` bytes, runs the compiled variant (C5, C5.hpp:282-474), returns the
  resized buffer or an ``Invalid`` status.
* ``pgnano::decompress_signal(compressed, pool, destination, state) -> Status``
  (pgnano.h:13-17, pgnano.cpp:98-126 -> C5.hpp:477-683).
* ``pod5_pinanoraw_compress_signal`` (c_api.cpp:1217-1253).
* the pod5 baseline codec VBZ, ``pod5::compress_signal`` / ``pod5::decompress_signal`` /
  ``pod5::compressed_signal_max_size`` (pod5/c++/pod5_format/signal_compression.cpp:14-141), as
  :class:`VBZCodec` with the same methods (the ``--VBZ`` side of the reference's copy tool).

``read_data`` / ``is_last_batch`` / ``state`` are accepted and ignored, exactly as C5 ignores them.
Errors raise :class:`PGNanoError` carrying the reference's status message.

The batched device API (:meth:`PGNanoCodec.compress_batch` / :meth:`decompress_batch`) takes
device-resident torch tensors: one launch encodes or decodes every chunk of a batch.
:meth:`PGNanoCodec.decompress_batch_pa` decodes straight to the calibrated signal a basecaller reads
(float32 or float16 pA; :func:`calibrate_signal` is the same arithmetic on the host).
:meth:`PGNanoCodec.decompress_reads_norm` decodes whole reads and writes each normalised by its own
quantiles or median / MAD; :meth:`PGNanoCodec.read_stats` gives those statistics for decoded reads.
:meth:`PGNanoCodec.segment_reads` trims the head of decoded reads, normalises them and cuts them into the
``[segments, length]`` tensor a model reads (:func:`trim_signal` and :func:`segment_signal` on the host).
:meth:`PGNanoCodec.stitch_plan` and :meth:`PGNanoCodec.stitch` undo that cut for the model's output: they drop
the frames doubled where rows overlap and lay each read's frames end to end (:func:`stitch_plan_signal` on the
host).  :meth:`PGNanoCodec.ctc_decode` turns those frames into bases by the best-path CTC rule, and
:meth:`PGNanoCodec.collapse_codes` is its second half for per-frame codes of any source
(:func:`ctc_decode_signal` and :func:`collapse_codes_signal` on the host).
:meth:`PGNanoCodec.crf_viterbi` is the decoder of CRF models: it turns the model's rows into such codes before
they are stitched (:func:`crf_viterbi_signal` on the host).

The host side of those stages -- every ``*_signal`` model, the ``*_bound`` functions and the ``*_params``
builders -- lives in :mod:`.host`, which needs NumPy alone.  This module holds the error type, the result
containers, the codecs and the plugin functions.  Every device call of :class:`PGNanoCodec` runs inside
:meth:`PGNanoCodec._launch`, where the stream contract is stated, and prepares its arguments with the helpers
below (:func:`_out_type`, :func:`_to`, :func:`_packed_offsets`, :func:`_reads_layout`, :func:`_require_out`).
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np

from . import _native
from .host import (_alphabet_bytes, _trim_struct, crf_params, ctc_params, norm_params, segment_bound, segment_params,
                   stitch_params)

MAX_CHUNK_SAMPLES = _native.PGN_MAX_CHUNK_SAMPLES


class PGNanoError(RuntimeError):
    """Mirrors the reference's ``arrow::Status::Invalid`` results."""

    def __init__(self, status: int, detail: str = ""):
        lib = _native.load()
        msg = lib.pgn_status_string(status).decode()
        if status == _native.PGN_ERR_HIP:
            msg += ": " + lib.pgn_last_error().decode()
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)
        self.status = status


def _check(rc: int, detail: str = "") -> None:
    if rc != _native.PGN_OK:
        raise PGNanoError(rc, detail)


def compressed_signal_max_size(sample_count: int) -> int:
    """``pgnano::Compressor::compressed_signal_max_size`` (compressor.h:39-45)."""
    return int(_native.load().pgn_compressed_signal_max_size(sample_count))


def _ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def _require_device(t, name: str, device: int) -> None:
    """The batch kernels dereference their data pointers on the GPU: a host tensor would fault."""
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{name} must be a tensor on cuda:{device} (got {t.device})")


def _require_out(t, name: str, device: int, dtype=None) -> None:
    """A destination or workspace the caller may pass: on the device and, where one is asked, of ``dtype``."""
    if t is not None:
        _require_device(t, name, device)
        if dtype is not None and t.dtype != dtype:
            raise ValueError(f"{name} must have dtype {dtype} (got {t.dtype})")


def _nreads(read_first_chunk) -> int:
    n = int(read_first_chunk.numel()) - 1
    if n < 0:
        raise ValueError("read_first_chunk needs nreads + 1 entries")
    return n


def _out_type(dtype, int16: bool = False) -> int:
    """The ``PGN_OUT_*`` value of a torch dtype: float32 or float16, and int16 where a call writes samples too."""
    import torch

    types = {torch.float32: _native.PGN_OUT_F32, torch.float16: _native.PGN_OUT_F16}
    if int16:
        types[torch.int16] = _native.PGN_OUT_INT16
    if dtype not in types:
        names = "torch.float32, torch.float16 or torch.int16" if int16 else "torch.float32 or torch.float16"
        raise ValueError(f"dtype must be {names} (got {dtype})")
    return types[dtype]


def _to(t, dev, dtype):
    """An argument as the kernels read it: on ``dev``, of ``dtype``, contiguous; None stays None."""
    return None if t is None else t.to(device=dev, dtype=dtype).contiguous()


def _crf_rows(rows, state_len, transitions, stay_score, time_major, device):
    """The rows argument of the CRF calls, checked: ``(pgn_crf_params, N, T, row dimension, frame dimension)``.
    ``transitions=None`` takes 4 or 5 from the frame's size."""
    import torch

    _require_device(rows, "rows", device)
    if rows.dim() != 3 or rows.dtype not in (torch.float16, torch.float32):
        raise ValueError("rows must be a [N, T, C] (or [T, N, C]) tensor of float16 or float32")
    nd, td = (1, 0) if time_major else (0, 1)
    N, T, C_ = int(rows.shape[nd]), int(rows.shape[td]), int(rows.shape[2])
    S = 4 ** int(state_len) if 1 <= int(state_len) <= 5 else 0
    if transitions is None:
        transitions = 4 if C_ == 4 * S else 5
    prm = crf_params(state_len, transitions, np.float16 if rows.dtype == torch.float16 else np.float32, stay_score)
    if C_ != prm.transitions * S:
        raise ValueError(f"rows must have {prm.transitions * S} scores per frame (got {C_})")
    if not 1 <= T <= _native.PGN_CRF_MAX_FRAMES:
        raise ValueError("rows must have between 1 and 2^24 frames")
    if rows.stride(2) != 1 or (T > 1 and rows.stride(td) < C_) or rows.stride(nd) < 0:
        raise ValueError("the last dimension of rows must be contiguous and the frame stride at least C")
    return prm, N, T, nd, td


def _packed_offsets(n: int, sizes):
    """Where each of ``n`` chunks starts when they lie end to end: the sum of the ``sizes`` (counts or
    capacities) before it, int64."""
    import torch

    offs = torch.zeros(n, dtype=torch.int64, device=sizes.device)
    if n > 1:
        offs[1:] = torch.cumsum(sizes.to(torch.int64), 0)[:-1]
    return offs


def _reads_layout(counts, first, read_out_offsets):
    """``(ends, read_out_offsets)`` of chunks in read order: ``ends[i]`` is the samples before chunk ``i``
    (chunks + 1 entries), and a read whose offset is not given starts where its first chunk would."""
    import torch

    ends = torch.zeros(int(counts.numel()) + 1, dtype=torch.int64, device=counts.device)
    ends[1:] = torch.cumsum(counts.to(torch.int64), 0)
    if read_out_offsets is None:
        return ends, ends[first[:-1]].contiguous()
    return ends, _to(read_out_offsets, counts.device, torch.int64)


def _chunk_arrays(blobs, blob_offsets, blob_sizes, sample_counts, out, out_offsets, dtype):
    """What both chunk decodes read, made on the launch stream: ``(counts, out_offsets, out, blob_offsets,
    blob_sizes)``.  Offsets that are not given are packed; an ``out`` that is not given is allocated for the sum of
    the counts, which waits for it on the host."""
    import torch

    dev = blobs.device
    counts = _to(sample_counts, dev, torch.int32)
    so = _packed_offsets(int(counts.numel()), counts) if out_offsets is None else _to(out_offsets, dev, torch.int64)
    if out is None:
        total = int(counts.to(torch.int64).sum().item())
        out = torch.empty(max(total, 1), dtype=dtype, device=dev)
    return counts, so, out, _to(blob_offsets, dev, torch.int64), _to(blob_sizes, dev, torch.int64)


def _read_arrays(blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, out, read_out_offsets, dtype):
    """What both reads decodes read, made on the launch stream: ``(counts, read_first_chunk, read_out_offsets,
    out, blob_offsets, blob_sizes)``.  Read offsets that are not given are packed; an ``out`` that is not given
    is allocated for the sum of the counts, which waits for it on the host."""
    import torch

    dev = blobs.device
    counts = _to(sample_counts, dev, torch.int32)
    first = _to(read_first_chunk, dev, torch.int64)
    ends, ro = _reads_layout(counts, first, read_out_offsets)
    if out is None:
        out = torch.empty(max(int(ends[-1].item()), 1), dtype=dtype, device=dev)
    return counts, first, ro, out, _to(blob_offsets, dev, torch.int64), _to(blob_sizes, dev, torch.int64)


class _Columns:
    """Named column views over one device tensor of C structs (``raw``: uint8, records x struct bytes): views,
    no copies; unsigned 32-bit fields come as int32 (their bits).  :meth:`numpy` gives the same as a structured
    host array."""

    DTYPE = None
    _COLS = {}

    def __init__(self, raw):
        self.raw = raw

    def __len__(self):
        return int(self.raw.shape[0])

    def __getattr__(self, name):
        import torch

        cols = type(self)._COLS
        if name in cols:
            t, col = cols[name]
            return self.raw.view(getattr(torch, t))[:, col]
        raise AttributeError(name)

    def numpy(self):
        return self.raw.cpu().numpy().reshape(-1).view(type(self).DTYPE)


class ReadStats(_Columns):
    """``pgn_read_stats`` of every read (``raw``: nreads x 32).  ``n`` int64, ``status`` int32, ``q_lo`` /
    ``q_hi`` int16, ``m2`` int32, ``mad4`` int32 (the uint32's bits; it stays below 2^18), ``centre`` /
    ``spread`` float32."""

    DTYPE = np.dtype([("n", "<u8"), ("status", "<i4"), ("q_lo", "<i2"), ("q_hi", "<i2"), ("m2", "<i4"),
                      ("mad4", "<u4"), ("centre", "<f4"), ("spread", "<f4")])
    _COLS = {"n": ("int64", 0), "status": ("int32", 2), "q_lo": ("int16", 6), "q_hi": ("int16", 7), "m2": ("int32", 4),
             "mad4": ("int32", 5), "centre": ("float32", 6), "spread": ("float32", 7)}


class ReadSegments(_Columns):
    """``pgn_read_segments`` of every read: ``first_segment`` int64, ``nsegments``, ``trim``, ``status``,
    ``head_m2``, ``head_mad4`` int32, ``threshold`` float32."""

    DTYPE = np.dtype([("first_segment", "<u8"), ("nsegments", "<u4"), ("trim", "<u4"), ("status", "<i4"),
                      ("head_m2", "<i4"), ("head_mad4", "<u4"), ("threshold", "<f4")])
    _COLS = {"first_segment": ("int64", 0), "nsegments": ("int32", 2), "trim": ("int32", 3), "status": ("int32", 4),
             "head_m2": ("int32", 5), "head_mad4": ("int32", 6), "threshold": ("float32", 7)}


class SegmentTable(_Columns):
    """``pgn_segment`` of every segment: ``read``, ``start`` (in the untrimmed read) and ``valid``, int32."""

    DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("valid", "<u4"), ("pad", "<u4")])
    _COLS = {"read": ("int32", 0), "start": ("int32", 1), "valid": ("int32", 2)}


@dataclass
class SegmentedReads:
    """What :meth:`PGNanoCodec.segment_reads` leaves on the device."""
    out: "object"       # [capacity, length] float16 / float32: rows [0, min(total, capacity)) are written
    segments: SegmentTable  # capacity entries, the same rows
    reads: ReadSegments     # one entry per read
    stats: ReadStats        # of the trimmed reads
    total: "object"     # int64 device scalar: the segments the batch needs


class StitchTable(_Columns):
    """``pgn_stitch_segment`` of every segment: frames ``[first, first + count)`` of the row are kept and go to
    frame ``dst_frame`` (int64) on; ``first`` and ``count`` int32."""

    DTYPE = np.dtype([("dst_frame", "<u8"), ("first", "<u4"), ("count", "<u4")])
    _COLS = {"dst_frame": ("int64", 0), "first": ("int32", 2), "count": ("int32", 3)}


@dataclass
class StitchPlan:
    """What :meth:`PGNanoCodec.stitch_plan` leaves on the device."""
    segments: StitchTable   # one entry per row of the segment table it was made from
    read_frames: "object"   # int64, reads + 1: read r's frames are [read_frames[r], read_frames[r + 1])
    params: "object"        # the pgn_stitch_params it was made with


@dataclass
class DecodedReads:
    """What :meth:`PGNanoCodec.ctc_decode` and :meth:`PGNanoCodec.collapse_codes` leave on the device."""
    seq: "object"         # uint8, capacity: read r's bases are seq[read_bases[r]:read_bases[r + 1]]; the entries
                          # of seq, base_frame and base_score from read_bases[-1] on are not initialised, nor are
                          # the codes of frames outside the taken reads
    read_bases: "object"  # int64, reads + 1: the full counts, also where the capacity cut the bases
    status: "object"      # int32 per read: 0, PGN_ERR_DST_TOO_SMALL (1) or PGN_ERR_INVALID_ARG (10, not taken)
    base_frame: "object"  # int32 per base (the uint32's bits): its frame within the read; or None
    base_score: "object"  # float32 per base: the winning score of its frame; or None
    codes: "object"       # uint8 per frame of the window: label, bit 7 set where the frame emits; or None
    params: "object"      # the pgn_ctc_params of a decode, the 128-entry alphabet of a collapse

    def sequences(self):
        """One ``bytes`` per read (waits on the host); a read the capacity cut gives the bases that fit."""
        seq, rb = self.seq.cpu().numpy(), self.read_bases.cpu().numpy()
        return [seq[a:b].tobytes() for a, b in zip(rb[:-1], rb[1:])]


@dataclass
class CrfCodes:
    """What :meth:`PGNanoCodec.crf_viterbi` leaves on the device."""
    codes: "object"      # uint8 [N, T]: the newest base of the frame's state, bit 7 set where the path moves
    row_score: "object"  # float32 [N]: the score of each row's best path; or None
    params: "object"     # the pgn_crf_params of the call


@dataclass
class EncodedBatch:
    blobs: "object"          # torch.uint8 device tensor holding every blob at its offset
    offsets: "object"        # torch.uint64 (as int64) blob offsets
    caps: "object"           # capacities used (compressed_signal_max_size per chunk)
    sizes: "object"          # blob sizes
    status: "object"         # int32 status per chunk
    stats: "object | None"   # (nchunks, 10) raw + frame sizes per stream


class PGNanoCodec:
    """One codec context per HIP device (one process per GPU)."""

    # C-ABI entry points of this codec
    _fn_compress, _fn_decompress = "pgn_compress_signal", "pgn_decompress_signal"
    _fn_compress_batch, _fn_decompress_batch = "pgn_compress_batch_device", "pgn_decompress_batch_device"

    @staticmethod
    def max_size(sample_count: int) -> int:
        return compressed_signal_max_size(sample_count)

    @staticmethod
    def _default_caps(counts):
        import torch

        return torch.clamp(counts.to(torch.int64) * 2 + 26, min=1024)

    def __init__(self, device: int = 0, variant: str = "C5"):
        """variant: the reference's compile-time COMPRESSOR_* choice (pgnano.cpp:70-92) as a runtime
        option -- "C5" (default, the reference default), "C4", "C1", "C2", "C3", "VBZ0"."""
        if variant not in _native.VARIANTS:
            raise ValueError(f"unknown pgnano variant {variant!r}; one of {sorted(_native.VARIANTS)}")
        self.variant = variant
        self._lib = _native.load()
        h = C.c_void_p()
        _check(self._lib.pgn_ctx_create(int(device), C.byref(h)), f"device {device}")
        self._h = h
        self.device = int(device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pgn_ctx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    _VARIANT_FN = {"pgn_compress_signal": "pgn_variant_compress_signal",
                   "pgn_decompress_signal": "pgn_variant_decompress_signal",
                   "pgn_compress_batch_device": "pgn_variant_compress_batch_device",
                   "pgn_decompress_batch_device": "pgn_variant_decompress_batch_device"}

    def _call(self, fn: str, *args):
        """C5 (and VBZ) through their own entry points; the other variants through pgn_variant_*."""
        if getattr(self, "variant", "C5") != "C5" and fn in self._VARIANT_FN:
            return getattr(self._lib, self._VARIANT_FN[fn])(self._h, _native.VARIANTS[self.variant], *args)
        return getattr(self._lib, fn)(self._h, *args)

    def _bounded(self, fn: str, bound: int, *args):
        """The C5 batch calls with a chunk-size bound (pgnano_hip.h *_bounded)."""
        if type(self) is not PGNanoCodec or getattr(self, "variant", "C5") != "C5":
            raise ValueError("max_chunk_samples: the bounded batch calls are C5's")
        return getattr(self._lib, fn)(self._h, bound, *args)

    @contextmanager
    def _launch(self, stream):
        """The scope every device call runs in; yields the HIP stream the call runs on (the caller's ``stream``,
        else the context's), made to wait for the caller's current stream.  The body runs with it as torch's
        current stream: the call's own allocations and fills are issued on it too, so they are ordered before
        the kernels and the caching allocator ties them to that stream.  On a normal exit the caller's current
        stream is made to wait for it (an event, no host sync), so the outputs are usable there like the results
        of any torch op.  An exception leaves without that wait: there are no outputs."""
        import torch

        caller = torch.cuda.current_stream()
        ls = torch.cuda.ExternalStream(int(stream) if stream else self.stream, device=torch.device("cuda", self.device))
        ls.wait_stream(caller)
        with torch.cuda.stream(ls):
            yield ls
        caller.wait_stream(ls)

    @property
    def stream(self) -> int:
        return int(self._lib.pgn_ctx_stream(self._h) or 0)

    # ---- long reads: the selection shared by several workgroups ---------------------------
    @property
    def select_split(self):
        """``(split_min_samples, part_samples, max_split_reads)`` of this context (pgn_ctx_get_select_split):
        a read above ``split_min_samples`` is selected in parts of about ``part_samples`` by several workgroups,
        at most ``max_split_reads`` reads per call (0: off).  The statistics do not depend on it."""
        s = _native.SelectSplit()
        _check(self._lib.pgn_ctx_get_select_split(self._h, C.byref(s)))
        return int(s.split_min_samples), int(s.part_samples), int(s.max_split_reads)

    def set_select_split(self, split_min_samples=None, part_samples=None, max_split_reads=None) -> None:
        """Change the settings of :attr:`select_split`; an argument left out keeps its value."""
        cur = self.select_split
        new = [cur[i] if v is None else int(v) for i, v in enumerate((split_min_samples, part_samples, max_split_reads))]
        if any(not 0 <= v < 1 << 32 for v in new):
            raise ValueError("the select_split settings are uint32")
        _check(self._lib.pgn_ctx_set_select_split(self._h, C.byref(_native.SelectSplit(*new, 0))))

    def select_split_counts(self) -> dict:
        """How the most recent selection of this context treated its reads (pgn_select_split_counts; waits for
        the context's last call): reads of one wave (``short``), of one workgroup (``whole``), ``split`` reads
        and their ``parts``, and the reads among ``whole`` that were long enough but found ``no_slot``.  All 0
        when the split is off."""
        out = (C.c_uint64 * 5)()
        _check(self._lib.pgn_select_split_counts(self._h, C.byref(out)))
        return dict(zip(("short", "whole", "split", "parts", "no_slot"), (int(v) for v in out)))

    # ---- per-chunk plugin surface (host memory) -------------------------------------------
    def compress_signal(self, samples, read_data=None, is_last_batch: bool = False) -> bytes:
        x = np.ascontiguousarray(samples, dtype=np.int16)
        cap = self.max_size(x.size)
        out = np.empty(cap, dtype=np.uint8)
        size = C.c_size_t(0)
        rc = self._call(self._fn_compress, x.ctypes.data, x.size, out.ctypes.data, cap, C.byref(size))
        if rc == _native.PGN_ERR_DST_TOO_SMALL:
            raise PGNanoError(rc, f"Destination size: {cap}, Required size: {size.value}")
        _check(rc)
        return out[: size.value].tobytes()

    def decompress_signal(self, compressed, destination=None, state=None, sample_count: int | None = None):
        src = np.frombuffer(bytes(compressed), dtype=np.uint8)
        if destination is None:
            if sample_count is None:
                raise ValueError("need a destination array or sample_count")
            destination = np.empty(int(sample_count), dtype=np.int16)
        if destination.dtype != np.int16 or not destination.flags.c_contiguous:
            raise ValueError("destination must be a contiguous int16 array")
        _check(self._call(self._fn_decompress, src.ctypes.data if src.size else 0, src.size, destination.ctypes.data,
                          destination.size))
        return destination

    # ---- batched device API -----------------------------------------------------------------
    def compress_batch(self, samples, sample_offsets, sample_counts, with_stats: bool = False,
                       out=None, out_offsets=None, out_caps=None, stream: int | None = None,
                       max_chunk_samples: int | None = None) -> EncodedBatch:
        """Encode every chunk of a device-resident batch in one launch.

        samples: int16 cuda tensor; sample_offsets: int64 tensor (elements); sample_counts: int32.
        Blobs land at ``out_offsets`` (default: packed with compressed_signal_max_size capacities).
        max_chunk_samples: the caller's bound on the chunk sizes (pgn_compress_batch_device_bounded:
        no host wait when it is at most 262,144).
        """
        import torch

        _require_device(samples, "samples", self.device)
        _require_out(out, "out", self.device)
        with self._launch(stream) as ls:
            dev = samples.device
            n = int(sample_counts.numel())
            counts = _to(sample_counts, dev, torch.int32)
            offs = _to(sample_offsets, dev, torch.int64)
            caps = self._default_caps(counts) if out_caps is None else _to(out_caps, dev, torch.int64)
            oo = _packed_offsets(n, caps) if out_offsets is None else _to(out_offsets, dev, torch.int64)
            if out is None:
                total = int((oo[-1] + caps[-1]).item()) if n else 0
                out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            sizes = torch.zeros(n, dtype=torch.int64, device=dev)
            status = torch.full((n,), -1, dtype=torch.int32, device=dev)
            stats = torch.zeros((n, _native.PGN_STATS_PER_CHUNK), dtype=torch.int64, device=dev) if with_stats else None
            args = (n, _ptr(samples), _ptr(offs), _ptr(counts), _ptr(out), _ptr(oo), _ptr(caps), _ptr(sizes),
                    _ptr(status), _ptr(stats), ls.cuda_stream)
            if max_chunk_samples is not None:
                _check(self._bounded("pgn_compress_batch_device_bounded", int(max_chunk_samples), *args))
            else:
                _check(self._call(self._fn_compress_batch, *args))
        return EncodedBatch(out, oo, caps, sizes, status, stats)

    def decompress_batch(self, blobs, blob_offsets, blob_sizes, sample_counts, out=None, out_offsets=None,
                         stream: int | None = None, max_chunk_samples: int | None = None):
        """Decode a device-resident batch; returns (samples int16 tensor, offsets, status).
        max_chunk_samples: as in :meth:`compress_batch` (pgn_decompress_batch_device_bounded)."""
        import torch

        _require_device(blobs, "blobs", self.device)
        _require_out(out, "out", self.device)
        n = int(sample_counts.numel())
        with self._launch(stream) as ls:
            counts, so, out, bo, bs = _chunk_arrays(blobs, blob_offsets, blob_sizes, sample_counts, out, out_offsets,
                                                    torch.int16)
            status = torch.full((n,), -1, dtype=torch.int32, device=blobs.device)
            args = (n, _ptr(blobs), _ptr(bo), _ptr(bs), _ptr(out), _ptr(so), _ptr(counts), _ptr(status), ls.cuda_stream)
            if max_chunk_samples is not None:
                _check(self._bounded("pgn_decompress_batch_device_bounded", int(max_chunk_samples), *args))
            else:
                _check(self._call(self._fn_decompress_batch, *args))
        return out, so, status

    @property
    def _pa_codec(self) -> int:
        """This codec's id for pgn_decompress_batch_device_pa (a pgn_variant value)."""
        return _native.VARIANTS[self.variant]

    def decompress_batch_pa(self, blobs, blob_offsets, blob_sizes, sample_counts, cal_offset, cal_scale,
                            dtype=None, out=None, out_offsets=None, stream: int | None = None,
                            max_chunk_samples: int | None = None):
        """Decode a device-resident batch straight to the calibrated signal; returns (out, offsets, status).

        The merge kernels write ``pA = (adc + offset) * scale`` themselves (pgn_decompress_batch_device_pa),
        so no second pass reads the int16 samples back.  dtype: ``torch.float32`` (default; exactly
        ``(adc.astype(float32) + float32(offset)) * float32(scale)``, the reference reader's
        ``calibrate_signal_array``), ``torch.float16`` (that value rounded once, to nearest even), or
        ``torch.int16`` (the samples :meth:`decompress_batch` writes).

        cal_offset, cal_scale: float32 tensors with one entry per chunk (ignored for int16, may be
        None).  Calibration belongs to a read, and the chunks of a read share it, so expand the reads'
        values with the chunks' read indices::

            cal_offset = cal_offset_read[read_index]    # read_index[i]: the read chunk i belongs to
            cal_scale = cal_scale_read[read_index]

        out / out_offsets: the destination (of ``dtype``, on the device) and the chunks' places in it,
        in elements.  stream and max_chunk_samples as in :meth:`decompress_batch`; here the bound is
        accepted for every codec and must be > 0 when given."""
        import torch

        dtype = torch.float32 if dtype is None else dtype
        out_type = _out_type(dtype, int16=True)
        if max_chunk_samples is not None and int(max_chunk_samples) <= 0:
            raise ValueError("max_chunk_samples must be > 0 when given (None: no bound)")
        _require_device(blobs, "blobs", self.device)
        n = int(sample_counts.numel())
        _require_out(out, "out", self.device, dtype)
        calibrated = dtype != torch.int16
        if calibrated:
            for t, name in ((cal_offset, "cal_offset"), (cal_scale, "cal_scale")):
                if t is None or int(t.numel()) != n:
                    raise ValueError(f"{name} must have one entry per chunk ({n})")
        with self._launch(stream) as ls:
            dev = blobs.device
            counts, so, out, bo, bs = _chunk_arrays(blobs, blob_offsets, blob_sizes, sample_counts, out, out_offsets, dtype)
            co = _to(cal_offset if calibrated else None, dev, torch.float32)
            cs = _to(cal_scale if calibrated else None, dev, torch.float32)
            status = torch.full((n,), -1, dtype=torch.int32, device=dev)
            _check(self._lib.pgn_decompress_batch_device_pa(
                self._h, self._pa_codec, int(max_chunk_samples or 0), n, _ptr(blobs), _ptr(bo), _ptr(bs), _ptr(out),
                out_type, _ptr(so), _ptr(counts), _ptr(co), _ptr(cs), _ptr(status), ls.cuda_stream))
        return out, so, status

    def read_stats(self, samples, read_offsets, read_counts, stream: int | None = None, **params) -> ReadStats:
        """The robust statistics of reads already decoded on the device (pgn_read_stats_device): read r is
        ``samples[read_offsets[r] : read_offsets[r] + read_counts[r]]`` (int16; any start).  params: ``mode``
        ("quantile" | "medmad"), ``p``, ``centre_mult``, ``spread_mult``, ``spread_floor`` as in
        :meth:`decompress_reads_norm`.  Exact: rank k = floor(p * (n - 1)) of the sorted read, the median and
        the MAD as numpy gives them in float64."""
        import torch

        prm = norm_params(**params)
        _require_device(samples, "samples", self.device)
        if samples.dtype != torch.int16:
            raise ValueError(f"samples must be int16 (got {samples.dtype})")
        with self._launch(stream) as ls:
            dev = samples.device
            n = int(read_counts.numel())
            ro, rc = _to(read_offsets, dev, torch.int64), _to(read_counts, dev, torch.int64)
            raw = torch.zeros((n, C.sizeof(_native.ReadStats)), dtype=torch.uint8, device=dev)
            _check(self._lib.pgn_read_stats_device(self._h, n, _ptr(samples), _ptr(ro), _ptr(rc), C.byref(prm),
                                                   _ptr(raw), ls.cuda_stream))
        return ReadStats(raw)

    def segment_reads(self, samples, read_offsets, read_counts, *, length, overlap, trim=None, dtype=None,
                      read_status=None, capacity=None, out=None, stream: int | None = None,
                      **norm) -> SegmentedReads:
        """Decoded reads on the device -> the model-input tensor (pgn_segment_reads_device): each read loses its
        trimmed head, is normalised by the statistics of what is left and cut into rows of ``length`` elements
        that overlap by ``overlap``; the last row of a read is aligned to its end and a short read is padded with
        +0.0.  Bit for bit what :func:`segment_signal` gives on the host, read after read.

        Read r is ``samples[read_offsets[r] : read_offsets[r] + read_counts[r]]`` (int16; any start); offsets and
        counts are tensors or host arrays.  trim: ``None`` / ``False`` for none, ``True`` for the usual head trim,
        or a dict for :func:`trim_params`.  dtype ``torch.float16`` (default) or ``torch.float32``.
        ``**norm`` as in :func:`norm_params`.  read_status: int32 per read (e.g. a loader's); a read whose entry
        is not 0 gives no segments and keeps that status.  capacity: rows of ``out`` (default: ``out``'s, else
        :func:`segment_bound` of the counts, which copies device counts to the host -- pass it, or host counts,
        to avoid that wait); segments beyond it are not written and their reads get status 1.  out: a
        contiguous ``[rows, length]`` tensor of ``dtype``.  No host wait in the call itself: ``total`` and every
        index stay on the device."""
        import torch

        dtype = torch.float16 if dtype is None else dtype
        out_type = _out_type(dtype)
        seg, prm, tprm = segment_params(length, overlap), norm_params(**norm), _trim_struct(trim)
        _require_device(samples, "samples", self.device)
        if samples.dtype != torch.int16:
            raise ValueError(f"samples must be int16 (got {samples.dtype})")
        if out is not None:
            _require_device(out, "out", self.device)
            if out.dtype != dtype or out.dim() != 2 or out.shape[1] != seg.length or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous [rows, {seg.length}] tensor of {dtype}")
            if capacity is not None and int(capacity) > out.shape[0]:
                raise ValueError(f"capacity {int(capacity)} is beyond out's {out.shape[0]} rows")
        if capacity is None:
            host = read_counts.cpu().numpy() if isinstance(read_counts, torch.Tensor) else read_counts
            capacity = out.shape[0] if out is not None else segment_bound(host, seg.length, seg.overlap)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        dev = samples.device

        def i64(a):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
            return _to(t, dev, torch.int64)

        with self._launch(stream) as ls:
            ro, rc = i64(read_offsets), i64(read_counts)
            n = int(rc.numel())
            if int(ro.numel()) != n:
                raise ValueError("read_offsets and read_counts must have one entry per read")
            st_in = _to(read_status, dev, torch.int32)
            if st_in is not None and int(st_in.numel()) != n:
                raise ValueError(f"read_status must have one entry per read ({n})")
            if out is None:
                out = torch.empty((capacity, seg.length), dtype=dtype, device=dev)
            segs = torch.zeros((capacity, C.sizeof(_native.Segment)), dtype=torch.uint8, device=dev)
            reads = torch.zeros((n, C.sizeof(_native.ReadSegments)), dtype=torch.uint8, device=dev)
            raw = torch.zeros((n, C.sizeof(_native.ReadStats)), dtype=torch.uint8, device=dev)
            total = torch.zeros((), dtype=torch.int64, device=dev)
            _check(self._lib.pgn_segment_reads_device(
                self._h, n, _ptr(samples), _ptr(ro), _ptr(rc), _ptr(st_in), C.byref(tprm), C.byref(prm), C.byref(seg),
                _ptr(out), out_type, capacity, _ptr(segs), _ptr(reads), _ptr(raw), _ptr(total), ls.cuda_stream))
        return SegmentedReads(out, SegmentTable(segs), ReadSegments(reads), ReadStats(raw), total)

    def stitch_plan(self, segmented: SegmentedReads, length, overlap, frame_samples, capacity=None,
                    stream: int | None = None) -> StitchPlan:
        """Which frames of a model's output for every row of ``segmented`` are kept, and where they go when the
        reads are laid end to end (pgn_stitch_plan_device): a model of stride ``frame_samples`` gives
        ``length // frame_samples`` frames per row, and rows of one read overlap.  ``length`` and ``overlap`` are
        the ones ``segmented`` was cut with.  Per read :func:`stitch_plan_signal` of its table rows; a read whose
        status is not 0 (or that the capacity cuts) gives no frames.  capacity: the rows of the segment table
        that may be read (default: all it has).  No host wait."""
        import torch

        prm = stitch_params(length, overlap, frame_samples)
        segs, reads = segmented.segments.raw, segmented.reads.raw
        _require_device(reads, "segmented.reads", self.device)
        _require_device(segs, "segmented.segments", self.device)
        if not (segs.is_contiguous() and reads.is_contiguous()):
            raise ValueError("the tables of segmented must be contiguous")
        capacity = int(segs.shape[0]) if capacity is None else int(capacity)
        if not 0 <= capacity <= int(segs.shape[0]):
            raise ValueError(f"capacity must lie in [0, {int(segs.shape[0])}], the rows of the segment table")
        n = int(reads.shape[0])
        with self._launch(stream) as ls:
            dev = reads.device
            plan = torch.zeros((capacity, C.sizeof(_native.StitchSegment)), dtype=torch.uint8, device=dev)
            frames = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            _check(self._lib.pgn_stitch_plan_device(self._h, n, _ptr(reads), _ptr(segs), capacity, C.byref(prm),
                                                    _ptr(plan), _ptr(frames), ls.cuda_stream))
        return StitchPlan(StitchTable(plan), frames, prm)

    def stitch(self, plan: StitchPlan, rows, first_segment: int = 0, out=None, frame_base: int = 0,
               time_major: bool = False, stream: int | None = None):
        """The kept frames of one model batch, copied to where ``plan`` puts them (pgn_stitch_rows_device).

        rows: the model's output for table rows ``[first_segment, first_segment + N)``, a tensor of any dtype,
        ``[N, T, ...]`` or with ``time_major`` ``[T, N, ...]``; the trailing dimensions form the frame and must
        be contiguous, the first two may have any strides.  out: ``[frames, ...]`` contiguous, of rows' dtype
        and frame shape; frame ``i`` of the stitched reads goes to ``out[i - frame_base]`` and a frame outside
        ``out`` is not written, so a batch may be stitched into a buffer of its own (``frame_base`` = its first
        ``dst_frame``) or all batches into one.  Without ``out`` one is allocated for every frame from
        ``frame_base`` on, which waits for ``plan.read_frames[-1]``.  Returns ``out``; nothing but kept
        frames is written to it."""
        import torch

        prm = plan.params
        T = prm.length // prm.frame_samples
        _require_device(rows, "rows", self.device)
        if rows.dim() < 2:
            raise ValueError("rows must have at least the two dimensions [N, T] (or [T, N])")
        nd, td = (1, 0) if time_major else (0, 1)
        N = int(rows.shape[nd])
        if int(rows.shape[td]) != T:
            raise ValueError(f"rows must have {T} frames per row (got {int(rows.shape[td])})")
        frame_shape = tuple(rows.shape[2:])
        item = rows.element_size()
        frame_bytes = item * int(np.prod(frame_shape, dtype=np.int64))
        if frame_bytes == 0:
            raise ValueError("a frame must have at least one element")
        expect = 1
        for size, stride in zip(reversed(frame_shape), reversed(rows.stride()[2:])):
            if size != 1 and stride != expect:
                raise ValueError("the trailing dimensions of rows (the frame) must be contiguous")
            expect *= size
        first_segment, frame_base = int(first_segment), int(frame_base)
        if first_segment < 0 or frame_base < 0 or first_segment + N > len(plan.segments):
            raise ValueError(f"rows [{first_segment}, {first_segment + N}) are not all in the plan's {len(plan.segments)}")
        if out is None:
            total = int(plan.read_frames[-1].item())
            out = torch.empty((max(total - frame_base, 0),) + frame_shape, dtype=rows.dtype, device=rows.device)
        else:
            _require_device(out, "out", self.device)
            if out.dtype != rows.dtype or tuple(out.shape[1:]) != frame_shape or out.dim() < 1 or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous [frames{''.join(', %d' % d for d in frame_shape)}] tensor of {rows.dtype}")
        with self._launch(stream) as ls:
            _check(self._lib.pgn_stitch_rows_device(
                self._h, C.byref(prm), _ptr(plan.segments.raw), first_segment, N, _ptr(rows), int(rows.stride(nd)) * item,
                int(rows.stride(td)) * item, frame_bytes, _ptr(out), frame_base, int(out.shape[0]), ls.cuda_stream))
        return out

    def _decode_outputs(self, read_frames, frames, capacity, base_frame, dev):
        """The arguments both base calls share, checked, and their output tensors (on the launch stream)."""
        import torch

        _require_device(read_frames, "read_frames", self.device)
        if read_frames.dtype != torch.int64 or read_frames.dim() != 1 or read_frames.numel() < 1 or not read_frames.is_contiguous():
            raise ValueError("read_frames must be a contiguous int64 tensor of reads + 1 offsets")
        capacity = frames if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        n = int(read_frames.numel()) - 1
        seq = torch.empty(capacity, dtype=torch.uint8, device=dev)
        bases = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        bf = torch.empty(capacity, dtype=torch.int32, device=dev) if base_frame else None
        return n, capacity, seq, bases, status, bf

    def ctc_decode(self, frames, read_frames, *, alphabet="NACGT", blank=0, frame_base: int = 0, capacity=None,
                   base_frame: bool = True, base_score: bool = True, codes: bool = False,
                   stream: int | None = None) -> DecodedReads:
        """The best-path CTC decode of stitched frames (pgn_ctc_decode_device): per read
        :func:`ctc_decode_signal` of its frames.

        frames: ``[F, C]`` float16 or float32, the last dimension contiguous, the first of any stride that is at
        least the frame; ``frames[i - frame_base]`` is frame ``i`` of the layout ``read_frames`` (int64, reads +
        1, as :meth:`stitch_plan` leaves it) describes.  A read that does not lie wholly in ``[frame_base,
        frame_base + F)`` gets status 10 and no bases.  capacity: the bases ``seq`` holds (default ``F``, which
        always suffices); reads cut by it get status 1, and ``read_bases`` still holds the full counts.
        ``base_frame`` / ``base_score`` / ``codes``: whether those outputs are made.  No host wait."""
        import torch

        _require_device(frames, "frames", self.device)
        if frames.dim() != 2 or frames.dtype not in (torch.float16, torch.float32):
            raise ValueError("frames must be a [F, C] tensor of float16 or float32")
        F, C_ = int(frames.shape[0]), int(frames.shape[1])
        prm = ctc_params(C_, blank, alphabet, np.float16 if frames.dtype == torch.float16 else np.float32)
        if frames.stride(1) != 1 or (F > 1 and frames.stride(0) < C_):
            raise ValueError("the last dimension of frames must be contiguous and the first stride at least C")
        frame_base = int(frame_base)
        if not 0 <= frame_base < 1 << 62:
            raise ValueError("frame_base must lie in [0, 2^62)")
        item = frames.element_size()
        stride = max(int(frames.stride(0)), C_) * item
        with self._launch(stream) as ls:
            dev = frames.device
            n, capacity, seq, bases, status, bf = self._decode_outputs(read_frames, F, capacity, base_frame, dev)
            bs = torch.empty(capacity, dtype=torch.float32, device=dev) if base_score else None
            cd = torch.empty(F, dtype=torch.uint8, device=dev) if codes else None
            _check(self._lib.pgn_ctc_decode_device(
                self._h, C.byref(prm), n, _ptr(read_frames), _ptr(frames) if F else 0, stride, frame_base, F, _ptr(seq),
                capacity, _ptr(bases), _ptr(status), _ptr(bf), _ptr(bs), _ptr(cd), ls.cuda_stream))
        return DecodedReads(seq, bases, status, bf, bs, cd, prm)

    def collapse_codes(self, codes, read_frames, alphabet, *, frame_base: int = 0, capacity=None,
                       base_frame: bool = True, stream: int | None = None) -> DecodedReads:
        """Code bytes to bases (pgn_collapse_codes_device), the second half of :meth:`ctc_decode` for codes of any
        source: per read :func:`collapse_codes_signal` of its codes.  codes: uint8, contiguous, ``codes[i -
        frame_base]`` for frame ``i``; alphabet: up to 128 bytes, the base of class ``code & 0x7f``.  The
        window, ``capacity`` and the statuses are those of :meth:`ctc_decode`.  No host wait."""
        import torch

        _require_device(codes, "codes", self.device)
        if codes.dtype != torch.uint8 or codes.dim() != 1 or not codes.is_contiguous():
            raise ValueError("codes must be a contiguous one-dimensional uint8 tensor")
        table = (C.c_uint8 * 128)(*_alphabet_bytes(alphabet, 128))
        frame_base, F = int(frame_base), int(codes.numel())
        if not 0 <= frame_base < 1 << 62:
            raise ValueError("frame_base must lie in [0, 2^62)")
        with self._launch(stream) as ls:
            n, capacity, seq, bases, status, bf = self._decode_outputs(read_frames, F, capacity, base_frame,
                                                                       codes.device)
            _check(self._lib.pgn_collapse_codes_device(
                self._h, C.byref(table), n, _ptr(read_frames), _ptr(codes) if F else 0, frame_base, F, _ptr(seq), capacity,
                _ptr(bases), _ptr(status), _ptr(bf), ls.cuda_stream))
        return DecodedReads(seq, bases, status, bf, None, codes, table)

    def set_crf_scratch(self, nbytes: int = 0) -> None:
        """The cap on the scratch of :meth:`crf_viterbi` (pgn_ctx_set_crf_scratch): the backpointers take
        ``4 * 4 ** state_len * ceil(T / 8) + 16`` bytes per row, and the rows of a call are decoded in groups that
        fit the cap.  0 restores the default, 1 GiB.  A call whose single row exceeds the cap is refused."""
        nbytes = int(nbytes)
        if not 0 <= nbytes < 1 << 64:
            raise ValueError("the scratch cap is a uint64")
        _check(self._lib.pgn_ctx_set_crf_scratch(self._h, nbytes))

    def crf_viterbi(self, rows, state_len, *, transitions=None, stay_score=0.0, time_major: bool = False, codes=None,
                    row_score: bool = True, stream: int | None = None) -> CrfCodes:
        """The best-path (Viterbi) decode of a CRF model's rows (pgn_crf_viterbi_rows_device): per row
        :func:`crf_viterbi_signal` of its scores.

        rows: the model's output for one batch, ``[N, T, C]`` or with ``time_major`` ``[T, N, C]``, float16 or
        float32, the last dimension contiguous, the other two of any strides (the frame stride at least ``C``);
        ``C`` is ``5 * 4 ** state_len`` or ``4 * 4 ** state_len``, which decides ``transitions`` when it is
        None.  codes: a uint8 ``[N, T]`` tensor to write into, its last dimension contiguous and its row stride at
        least ``T`` (default: a new one).  ``row_score``: whether the rows' path scores are made.  No host wait.

        The codes are the bytes :meth:`collapse_codes` reads, and :meth:`stitch` moves one-byte frames, so for
        table rows ``[first_segment, first_segment + N)`` of a segmented batch::

            result = codec.crf_viterbi(model(rows), state_len)
            frames = codec.stitch(plan, result.codes, first_segment, out=frames)
            bases = codec.collapse_codes(frames, plan.read_frames, "ACGT")
        """
        import torch

        prm, N, T, nd, td = _crf_rows(rows, state_len, transitions, stay_score, time_major, self.device)
        item = rows.element_size()
        with self._launch(stream) as ls:
            if codes is None:
                codes = torch.empty((N, T), dtype=torch.uint8, device=rows.device)
            else:
                _require_device(codes, "codes", self.device)
                if (codes.dtype != torch.uint8 or tuple(codes.shape) != (N, T) or (T > 1 and codes.stride(1) != 1)
                        or (N > 1 and codes.stride(0) < T)):
                    raise ValueError(f"codes must be a uint8 [{N}, {T}] tensor, rows contiguous and at least T apart")
            score = torch.empty(N, dtype=torch.float32, device=rows.device) if row_score else None
            if N:
                _check(self._lib.pgn_crf_viterbi_rows_device(
                    self._h, C.byref(prm), N, T, _ptr(rows), int(rows.stride(nd)) * item, int(rows.stride(td)) * item,
                    _ptr(codes), max(int(codes.stride(0)), T) if N > 1 else T, _ptr(score), ls.cuda_stream))
        return CrfCodes(codes, score, prm)

    def decompress_reads_norm(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, *,
                              mode="quantile", p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, spread_floor=1.0,
                              dtype=None, out=None, read_out_offsets=None, adc=None, max_chunk_samples: int = 0,
                              stream: int | None = None):
        """Decode whole reads and write each normalised by its own statistics, contiguous; returns
        (out, read_out_offsets, :class:`ReadStats`, chunk statuses).

        The chunks are in read order and ``read_first_chunk`` (nreads + 1 entries) says which are whose: read r
        owns chunks ``read_first_chunk[r] : read_first_chunk[r + 1]``.  mode "quantile": with a, b the
        samples of rank ``floor(p * (n - 1))`` for ``p = (p_lo, p_hi)``, ``centre = centre_mult * (a + b)``
        and ``spread = spread_mult * (b - a)``; mode "medmad": ``centre = median``, ``spread = spread_mult *
        MAD``.  ``spread`` is at least ``spread_floor``; the output is ``(adc + (-centre)) * (1 / spread)``
        in float32 (``dtype=torch.float32``), or that rounded once to float16 (the default).  Bit for bit
        what :func:`normalise_signal` gives on the host.

        out / read_out_offsets: the destination (of ``dtype``) and each read's first element in it (default:
        packed).  adc: an int16 tensor that receives the raw samples at the same element offsets; without
        it float16 is converted in place and float32 takes a workspace allocated here.  max_chunk_samples:
        the caller's bound on the chunk sizes, 0 for none.  A read's ``status`` is its first failing chunk's."""
        import torch

        dtype = torch.float16 if dtype is None else dtype
        out_type = _out_type(dtype)
        prm = norm_params(mode, p, centre_mult, spread_mult, spread_floor)
        if int(max_chunk_samples) < 0:
            raise ValueError("max_chunk_samples must be >= 0 (0: no bound)")
        _require_device(blobs, "blobs", self.device)
        nchunks, nreads = int(sample_counts.numel()), _nreads(read_first_chunk)
        _require_out(out, "out", self.device, dtype)
        _require_out(adc, "adc", self.device, torch.int16)
        with self._launch(stream) as ls:
            dev = blobs.device
            counts, first, ro, out, bo, bs = _read_arrays(blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk,
                                                          out, read_out_offsets, dtype)
            if adc is None and dtype == torch.float32:
                work = torch.empty(out.numel(), dtype=torch.int16, device=dev)
            else:
                work = adc
            status = torch.full((nchunks,), -1, dtype=torch.int32, device=dev)
            raw = torch.zeros((nreads, C.sizeof(_native.ReadStats)), dtype=torch.uint8, device=dev)
            _check(self._lib.pgn_decompress_reads_device_norm(
                self._h, self._pa_codec, int(max_chunk_samples), nreads, nchunks, _ptr(first), _ptr(blobs), _ptr(bo),
                _ptr(bs), _ptr(counts), _ptr(out), out_type, _ptr(ro), _ptr(work), C.byref(prm), _ptr(raw),
                _ptr(status), ls.cuda_stream))
        return out, ro, ReadStats(raw), status

    def decompress_reads_pa(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, cal_offset=None,
                            cal_scale=None, *, dtype=None, out=None, read_out_offsets=None, max_chunk_samples: int = 0,
                            stream: int | None = None):
        """Decode whole reads straight to the calibrated signal, each read contiguous; returns
        (out, read_out_offsets, read statuses, chunk statuses).

        The reads-shaped :meth:`decompress_batch_pa` (pgn_decompress_reads_device_pa): the chunks are in read
        order, ``read_first_chunk`` (nreads + 1 entries) says which are whose, and ``cal_offset`` /
        ``cal_scale`` have one float32 entry per **read** (ignored, may be None, for ``dtype=torch.int16``,
        which gives the reads' ADC counts).  dtype ``torch.float32`` (default), ``torch.float16`` or
        ``torch.int16``: the values are :meth:`decompress_batch_pa`'s bit for bit.  out / read_out_offsets: the
        destination (of ``dtype``) and each read's first element in it (default: packed).
        max_chunk_samples: the caller's bound on the chunk sizes, 0 for none.  A read's status is its first
        chunk status that is not 0, in chunk order (0 for a read without chunks)."""
        import torch

        dtype = torch.float32 if dtype is None else dtype
        out_type = _out_type(dtype, int16=True)
        if int(max_chunk_samples) < 0:
            raise ValueError("max_chunk_samples must be >= 0 (0: no bound)")
        _require_device(blobs, "blobs", self.device)
        nchunks, nreads = int(sample_counts.numel()), _nreads(read_first_chunk)
        _require_out(out, "out", self.device, dtype)
        calibrated = dtype != torch.int16
        if calibrated:
            for t, name in ((cal_offset, "cal_offset"), (cal_scale, "cal_scale")):
                if t is None or int(t.numel()) != nreads:
                    raise ValueError(f"{name} must have one entry per read ({nreads})")
        with self._launch(stream) as ls:
            dev = blobs.device
            counts, first, ro, out, bo, bs = _read_arrays(blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk,
                                                          out, read_out_offsets, dtype)
            co = _to(cal_offset if calibrated else None, dev, torch.float32)
            cs = _to(cal_scale if calibrated else None, dev, torch.float32)
            status = torch.full((nchunks,), -1, dtype=torch.int32, device=dev)
            read_status = torch.full((nreads,), -1, dtype=torch.int32, device=dev)
            _check(self._lib.pgn_decompress_reads_device_pa(
                self._h, self._pa_codec, int(max_chunk_samples), nreads, nchunks, _ptr(first), _ptr(blobs), _ptr(bo),
                _ptr(bs), _ptr(counts), _ptr(out), out_type, _ptr(ro), _ptr(co), _ptr(cs), _ptr(read_status),
                _ptr(status), ls.cuda_stream))
        return out, ro, read_status, status

    def reads_status(self, read_first_chunk, chunk_status, stream: int | None = None):
        """Each read's first chunk status that is not 0, in chunk order (pgn_reads_status_device): the
        per-read statuses for :meth:`decompress_reads_norm`'s chunk statuses."""
        import torch

        _require_device(chunk_status, "chunk_status", self.device)
        nreads = _nreads(read_first_chunk)
        with self._launch(stream) as ls:
            dev = chunk_status.device
            first, cs = _to(read_first_chunk, dev, torch.int64), _to(chunk_status, dev, torch.int32)
            out = torch.full((nreads,), -1, dtype=torch.int32, device=dev)
            _check(self._lib.pgn_reads_status_device(self._h, nreads, _ptr(first), _ptr(cs), _ptr(out), ls.cuda_stream))
        return out

    def synth_reads(self, nreads: int, samples_per_read, seed: int = 42, first_read: int = 0, read_stride: int = 1,
                    p_switch_q16: int = 6554, level_mean: int = 500, level_sd: int = 60, noise_sd: int = 12,
                    out=None):
        """Generate synthetic reads on the device (bench input); returns (samples, offsets, counts)."""
        import torch

        dev = torch.device("cuda", self.device)
        if isinstance(samples_per_read, int):
            counts = torch.full((nreads,), samples_per_read, dtype=torch.int32, device=dev)
        else:
            counts = torch.as_tensor(samples_per_read, dtype=torch.int32, device=dev)
        offs = _packed_offsets(nreads, counts)
        total = int(counts.to(torch.int64).sum().item())
        if out is None:
            out = torch.empty(max(total, 1), dtype=torch.int16, device=dev)
        _check(self._lib.pgn_synth_reads_device(self._h, nreads, seed, first_read, read_stride, _ptr(out), _ptr(offs),
                                                _ptr(counts), p_switch_q16, level_mean, level_sd, noise_sd, 0))
        return out, offs, counts

    def kernels(self, direction: int) -> str:
        """Kernel names of the C5 batch path (0 = encode, 1 = decode)."""
        return self._lib.pgn_ctx_kernels(self._h, int(direction)).decode()

    def last_encode_ms(self) -> float:
        return float(self._lib.pgn_ctx_last_encode_ms(self._h))

    def last_decode_ms(self) -> float:
        return float(self._lib.pgn_ctx_last_decode_ms(self._h))


def vbz_compressed_signal_max_size(sample_count: int) -> int:
    """``pod5::compressed_signal_max_size`` (signal_compression.cpp:14-19)."""
    return int(_native.load().pgn_vbz_compressed_signal_max_size(sample_count))


class VBZCodec(PGNanoCodec):
    """The pod5 VBZ codec (svb16 + zstd level 1) on the GPU: ``pod5::compress_signal`` /
    ``pod5::decompress_signal`` (signal_compression.cpp:21-141), same methods as
    :class:`PGNanoCodec`.  A frame larger than the destination raises "Failed to compress data"."""

    _fn_compress, _fn_decompress = "pgn_vbz_compress_signal", "pgn_vbz_decompress_signal"
    _fn_compress_batch, _fn_decompress_batch = "pgn_vbz_compress_batch_device", "pgn_vbz_decompress_batch_device"

    def __init__(self, device: int = 0):
        super().__init__(device)

    @property
    def _pa_codec(self) -> int:
        return _native.PGN_POD5_CODEC_VBZ

    @staticmethod
    def max_size(sample_count: int) -> int:
        return vbz_compressed_signal_max_size(sample_count)

    @staticmethod
    def _default_caps(counts):
        import torch

        c = counts.to(torch.int64)
        svb = (c >> 3) + (((c & 7) + 7) >> 3) + 2 * c
        small = (svb < 128 * 1024).to(torch.int64)
        return svb + (svb >> 8) + small * ((128 * 1024 - svb).clamp(min=0) >> 11)


_default: PGNanoCodec | None = None


def default_codec() -> PGNanoCodec:
    global _default
    if _default is None:
        _default = PGNanoCodec(0)
    return _default


def compress_signal(samples, pool=None, read_data=None, is_last_batch: bool = False) -> bytes:
    """Module-level ``pgnano::compress_signal`` on the default device."""
    return default_codec().compress_signal(samples, read_data, is_last_batch)


def decompress_signal(compressed, pool=None, destination=None, state=None, sample_count: int | None = None):
    """Module-level ``pgnano::decompress_signal`` on the default device."""
    return default_codec().decompress_signal(compressed, destination, state, sample_count)


def pinanoraw_compress_signal(signal, buffer_size: int | None = None) -> bytes:
    """``pod5_pinanoraw_compress_signal`` (c_api.cpp:1217-1253)."""
    lib = _native.load()
    x = np.ascontiguousarray(signal, dtype=np.int16)
    cap = buffer_size if buffer_size is not None else compressed_signal_max_size(x.size)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    size = C.c_size_t(cap)
    _check(lib.pgn_pinanoraw_compress_signal(x.ctypes.data, x.size, out.ctypes.data, C.byref(size)))
    return out[: size.value].tobytes()


def vbz_compress_signal_capi(signal, buffer_size: int | None = None) -> bytes:
    """``pod5_vbz_compress_signal`` (c_api.cpp:1183-1214): the --VBZ codec through the C-API shape."""
    lib = _native.load()
    x = np.ascontiguousarray(signal, dtype=np.int16)
    cap = buffer_size if buffer_size is not None else vbz_compressed_signal_max_size(x.size)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    size = C.c_size_t(cap)
    _check(lib.pgn_pod5_vbz_compress_signal(x.ctypes.data, x.size, out.ctypes.data, C.byref(size)))
    return out[: size.value].tobytes()


def vbz_decompress_signal_capi(compressed, sample_count: int):
    """``pod5_vbz_decompress_signal`` (c_api.cpp:1255-1273)."""
    lib = _native.load()
    src = np.frombuffer(bytes(compressed), dtype=np.uint8)
    out = np.empty(max(int(sample_count), 1), dtype=np.int16)
    _check(lib.pgn_pod5_vbz_decompress_signal(src.ctypes.data if src.size else 0, src.size, int(sample_count),
                                              out.ctypes.data))
    return out[: int(sample_count)]


class Pod5SignalBatch:
    """The batched POD5 signal-table integration (include/pgnano_pod5.h) on a codec's context.

    ``compress_reads(reads)`` is the signal half of ``pod5_add_reads_data`` (c_api.cpp:1104-1129):
    every read is chunked at ``chunk_size`` as the writer does (file_writer.cpp:119-143) and all
    chunks are compressed by one batched launch; it returns the signal column the writer appends
    (``offsets``, ``data``) with the per-chunk ``samples`` and ``read_index``.
    ``decompress_rows(offsets, data, samples)`` decodes a record batch of signal rows
    (signal_table_reader.cpp:294-318) into one int16 array."""

    def __init__(self, codec: PGNanoCodec, chunk_size: int = 0):
        self._codec = codec
        self._lib = codec._lib
        if isinstance(codec, VBZCodec):
            cid = _native.PGN_POD5_CODEC_VBZ
        else:
            cid = _native.VARIANTS[codec.variant]
        h = C.c_void_p()
        _check(self._lib.pgn_pod5_batch_create(codec._h, cid, int(chunk_size), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pgn_pod5_batch_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def compress_reads(self, reads, copy: bool = True):
        """(offsets, data, samples, read_index) of the chunked, compressed reads.  copy=False returns
        views of the batch's own buffers, valid until its next call (as in the C API)."""
        xs = [np.ascontiguousarray(r, dtype=np.int16) for r in reads]
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data if x.size else None for x in xs])
        sizes = np.array([x.size for x in xs] or [0], dtype=np.uint32)
        n = C.c_size_t(0)
        po, pd, ps, pr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self._lib.pgn_pod5_compress_reads(self._h, len(xs), ptrs, sizes.ctypes.data, C.byref(n), C.byref(po),
                                               C.byref(pd), C.byref(ps), C.byref(pr))
        _check(rc, f"chunk {n.value}" if rc else "")
        k = n.value
        cp = (lambda a: a.copy()) if copy else (lambda a: a)
        offsets = cp(np.ctypeslib.as_array((C.c_uint64 * (k + 1)).from_address(po.value)))
        data = (cp(np.ctypeslib.as_array((C.c_uint8 * int(offsets[-1])).from_address(pd.value)))
                if offsets[-1] else np.zeros(0, np.uint8))
        samples = cp(np.ctypeslib.as_array((C.c_uint32 * k).from_address(ps.value))) if k else np.zeros(0, np.uint32)
        read_index = cp(np.ctypeslib.as_array((C.c_uint32 * k).from_address(pr.value))) if k else np.zeros(0, np.uint32)
        return offsets, data, samples, read_index

    def decompress_rows(self, offsets, data, samples, out=None):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        k = samples.size
        # pgn_pod5_decompress_rows reads offsets[k] and the bytes offsets[0] .. offsets[k]
        if offsets.size != k + 1:
            raise ValueError(f"offsets has {offsets.size} entries, expected rows + 1 = {k + 1}")
        if k and (int(offsets[-1]) > data.size or np.any(np.diff(offsets.astype(np.int64)) < 0)):
            raise ValueError("offsets are not monotonic or run past the data buffer")
        total = int(samples.sum())
        if out is None:
            out = np.empty(max(total, 1), dtype=np.int16)
        elif out.dtype != np.int16 or not out.flags.c_contiguous or out.size < total:
            raise ValueError("out must be a contiguous int16 array of at least sum(samples) entries")
        st = np.zeros(max(k, 1), dtype=np.int32)
        _check(self._lib.pgn_pod5_decompress_rows(self._h, k, offsets.ctypes.data, data.ctypes.data if data.size else None,
                                                  samples.ctypes.data, out.ctypes.data, st.ctypes.data))
        return out[:total]
