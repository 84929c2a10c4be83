"""FASTQ records on the device (include/pgnano_hip.h, "FASTQ records"): a read's mean quality with a pass flag,
and the kept reads laid out as FASTQ text in one device buffer, as functions that take the codec.

The package's ``__all__`` and the methods of :class:`~rawnanoporesignalcompression_amd.codec.PGNanoCodec` are a
fixed surface, so the two device calls live here, like those of :mod:`~rawnanoporesignalcompression_amd.quality`,
whose route they finish::

    bases = codec.collapse_codes(frame_codes, plan.read_frames, "ACGT")
    qual = quality.base_qual(codec, bases, frame_codes, frame_post, plan.read_frames)
    rq = fastq.read_qual(codec, bases, qual, min_mean_q=9)
    ids, ch, rn = fastq.read_tags(pod5.reads(), reads, codec.device)
    rec = fastq.fastq_records(codec, bases, qual, ids, {"qs": rq.mean_q, "ch": ch, "rn": rn}, keep=rq.passed)
    with open(path, "wb") as f:
        f.write(rec.tobytes())                                   # the one host wait

The host models (:func:`read_qual_signal`, :func:`fastq_records_signal`, :func:`err_table`, :func:`fastq_bound`)
are those of :mod:`~rawnanoporesignalcompression_amd.host`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native
from . import tags as _tags
from .codec import DecodedReads, PGNanoCodec, _check, _ptr, _require_device, _require_out
from .host import (_fastq_tags, err_table, fastq_bound, fastq_bound_tagged, fastq_records_signal, read_qual_params,
                   read_qual_signal)

__all__ = ["read_qual", "fastq_records", "read_tags", "ReadQual", "FastqRecords", "read_qual_signal",
           "fastq_records_signal", "err_table", "fastq_bound"]


@dataclass
class ReadQual:
    """What :func:`read_qual` leaves on the device, an entry per read; all zero for a read without input."""
    mean_q: "object"   # int32 (the uint32's bits): q_min plus the thresholds the read's mean error does not exceed
    err_sum: "object"  # int64 (the uint64's bits): the sum of its counted bases' errors in units of 2^-32
    passed: "object"   # uint8: 1 where mean_q >= min_mean_q


@dataclass
class FastqRecords:
    """What :func:`fastq_records` leaves on the device."""
    data: "object"     # uint8: read r's record is data[rec_off[r]:rec_off[r + 1]] where status[r] is 0
    rec_off: "object"  # int64, reads + 1: the scan of all records' lengths; rec_off[-1] is the capacity that suffices
    status: "object"   # int32 per read: 0, PGN_ERR_DST_TOO_SMALL (1) for a record data could not hold, or the
                       # read's own status where it has no record

    def tobytes(self) -> bytes:
        """The text, ``data[:min(rec_off[-1], capacity)]`` (waits on the host: the one wait of the route).  Where
        ``data`` was too small for every record (a status of 1), the bytes behind the last written record are not
        text: such a caller cuts at the largest ``rec_off`` value within the capacity."""
        end = min(int(self.rec_off[-1].item()), int(self.data.numel()))
        return self.data[:end].cpu().numpy().tobytes()


def _read_arrays(codec, decoded, qual):
    """The reads' offsets, statuses and the base capacity of a record or mean call, checked."""
    import torch

    n = int(decoded.status.numel())
    for name, t, size, dtype in (("read_bases", decoded.read_bases, n + 1, torch.int64), ("status", decoded.status, n, torch.int32)):
        _require_device(t, f"decoded.{name}", codec.device)
        if t.dtype != dtype or int(t.numel()) != size or not t.is_contiguous():
            raise ValueError(f"decoded.{name} must hold {size} contiguous {dtype} entries")
    capacity = int(decoded.seq.numel())
    _require_device(qual, "qual", codec.device)
    if qual.dtype != torch.uint8 or qual.dim() != 1 or int(qual.numel()) != capacity or not qual.is_contiguous():
        raise ValueError(f"qual must be a contiguous uint8 tensor of {capacity} bytes, as decoded.seq")
    return n, capacity


def read_qual(codec: PGNanoCodec, decoded: DecodedReads, qual, thresholds=None, *, q_min: int = 1, skip_bases: int = 60,
              min_mean_q: int = 0, stream: int | None = None) -> ReadQual:
    """Mean quality and pass flag of every read (pgn_read_qual_device): :func:`read_qual_signal` of ``qual``,
    ``decoded.read_bases`` and ``decoded.status``, bit for bit, with :func:`err_table`.

    decoded: what :meth:`PGNanoCodec.collapse_codes` returned; qual: what :func:`quality.base_qual
    <rawnanoporesignalcompression_amd.quality.base_qual>` wrote for it.  thresholds and ``q_min`` are those of
    ``base_qual`` (default :func:`qual_thresholds <rawnanoporesignalcompression_amd.host.qual_thresholds>` from
    ``q_min`` to 50), applied to the mean error of the read's bases behind its first ``skip_bases``; a read passes
    with ``mean_q >= min_mean_q``.  No host wait."""
    import torch

    n, capacity = _read_arrays(codec, decoded, qual)
    prm = read_qual_params(thresholds, q_min, skip_bases, min_mean_q)
    with codec._launch(stream) as ls:
        dev = qual.device
        mean_q = torch.empty(n, dtype=torch.int32, device=dev)
        err_sum = torch.empty(n, dtype=torch.int64, device=dev)
        passed = torch.empty(n, dtype=torch.uint8, device=dev)
        _check(codec._lib.pgn_read_qual_device(
            codec._h, C.byref(prm), n, _ptr(decoded.read_bases), _ptr(decoded.status), _ptr(qual) if capacity else 0,
            capacity, _ptr(mean_q), _ptr(err_sum), _ptr(passed), ls.cuda_stream))
    return ReadQual(mean_q, err_sum, passed)


def fastq_records(codec: PGNanoCodec, decoded: DecodedReads, qual, read_ids, tags=None, *, keep=None, reverse: bool = False,
                  out=None, stream: int | None = None) -> FastqRecords:
    """The kept reads as FASTQ text (pgn_fastq_records_device): :func:`fastq_records_signal`, bit for bit.

    decoded and qual as for :func:`read_qual`; ``decoded.seq`` is the second line of a record and ``qual`` the
    fourth.  read_ids: a uint8 ``[reads, 16]`` device tensor, the uuids' bytes.  tags: a dict of two-character name
    to a device tensor of one 32-bit value per read (read as uint32), written as ``\\tXX:i:value`` in insertion
    order, at most 8.  With a typed column of :mod:`~rawnanoporesignalcompression_amd.tags` among the values
    (``tags.i32``, ``tags.zdict``, ``tags.zstr``, :func:`demux.barcode_tag
    <rawnanoporesignalcompression_amd.demux.barcode_tag>`; ``tags.f32`` is a ``ValueError``, a float has no text
    rule) the call is pgn_fastq_records_tagged_device, :func:`fastq_records_tagged_signal
    <rawnanoporesignalcompression_amd.host.fastq_records_tagged_signal>` bit for bit, with at most 16 columns.  keep: a uint8 or bool device tensor, a read with 0 gets no record (default: every read with
    bases does); ``ReadQual.passed`` writes the pass file and its complement the fail file.  reverse: both strings
    backwards.  out: a one-dimensional uint8 tensor to write into, any alignment (default: a new one of
    :func:`fastq_bound` bytes, which always suffices).  No host wait; :meth:`FastqRecords.tobytes` is the one."""
    import torch

    n, capacity = _read_arrays(codec, decoded, qual)
    _require_device(decoded.seq, "decoded.seq", codec.device)
    if decoded.seq.dtype != torch.uint8 or not decoded.seq.is_contiguous():
        raise ValueError("decoded.seq must be a contiguous uint8 tensor")
    _require_device(read_ids, "read_ids", codec.device)
    if read_ids.dtype != torch.uint8 or tuple(read_ids.shape) != (n, 16) or not read_ids.is_contiguous():
        raise ValueError(f"read_ids must be a contiguous uint8 [{n}, 16] tensor")
    typed = _tags.has_typed(tags)
    items = [] if typed else list((tags or {}).items())
    _fastq_tags([(name, ()) for name, _ in items], 0)       # the names and their number
    columns, typed_cols = _tags.native_columns(codec, tags, n, text=True) if typed else (None, ())
    prm = _native.FastqParams(_native.PGN_FASTQ_REVERSE if reverse else 0, len(items))
    for k, (name, t) in enumerate(items):
        _require_device(t, f"tags[{name!r}]", codec.device)
        if t.element_size() != 4 or t.is_floating_point() or int(t.numel()) != n or not t.is_contiguous():
            raise ValueError(f"tags[{name!r}] must hold {n} contiguous 32-bit integers")
        prm.tag_name[k][:] = list(name.encode("ascii"))
        prm.d_tag[k] = _ptr(t) if n else 0
    if keep is not None:
        _require_device(keep, "keep", codec.device)
        if keep.element_size() != 1 or int(keep.numel()) != n or not keep.is_contiguous():
            raise ValueError(f"keep must hold {n} contiguous bytes")
    with codec._launch(stream) as ls:
        dev = qual.device
        if out is None:
            bound = fastq_bound_tagged(n, capacity, typed_cols) if typed else fastq_bound(n, capacity, len(items))
            out = torch.empty(bound, dtype=torch.uint8, device=dev)
        else:
            _require_out(out, "out", codec.device, torch.uint8)
            if out.dim() != 1 or not out.is_contiguous():
                raise ValueError("out must be a contiguous one-dimensional uint8 tensor")
        rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        nbytes = int(out.numel())
        if typed:
            tagged = codec._lib.pgn_fastq_records_tagged_device
            call = lambda h, p, *rest: tagged(h, p, C.byref(columns), *rest)
        else:
            call = codec._lib.pgn_fastq_records_device
        _check(call(
            codec._h, C.byref(prm), n, _ptr(read_ids) if n else 0, _ptr(decoded.read_bases), _ptr(decoded.status),
            _ptr(keep) if keep is not None and n else 0, _ptr(decoded.seq) if capacity else 0,
            _ptr(qual) if capacity else 0, capacity, _ptr(out) if nbytes else 0, nbytes, _ptr(rec_off),
            _ptr(status) if n else 0, ls.cuda_stream))
    return FastqRecords(out, rec_off, status)


def read_tags(reads_table, reads, device):
    """``(read_id, ch, rn)`` of a selection from :meth:`Pod5File.reads
    <rawnanoporesignalcompression_amd.pod5_file.Pod5File.reads>` as device tensors: the uuids' bytes ``[reads,
    16]`` uint8, and the channels and read numbers as int32 (the uint32s' bits), ready to be the ``read_ids`` and
    the ``ch`` and ``rn`` tags of :func:`fastq_records`.  reads: indices into the table (None: all of it)."""
    import torch

    idx = slice(None) if reads is None else np.asarray(reads, dtype=np.int64).reshape(-1)
    dev = torch.device("cuda", int(device)) if isinstance(device, int) else torch.device(device)
    ids = np.ascontiguousarray(np.asarray(reads_table.read_id, dtype=np.uint8).reshape(-1, 16)[idx])
    col = lambda a: torch.from_numpy(np.asarray(a)[idx].astype(np.uint32).view(np.int32).copy()).to(dev)
    return torch.from_numpy(ids).to(dev), col(reads_table.channel), col(reads_table.read_number)
