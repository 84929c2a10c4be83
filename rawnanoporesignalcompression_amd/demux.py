"""Adapters and barcodes on the device (include/pgnano_hip.h, "Adapters and barcodes"): where the adapter, primer
and barcode sequences lie at the two ends of each read, which barcode a read carries, and the reads cut to what
lies between, with their qualities and move tables, as functions that take the codec.

The package's ``__all__`` and the methods of :class:`~rawnanoporesignalcompression_amd.codec.PGNanoCodec` are a
fixed surface, so the calls live here, like those of :mod:`~rawnanoporesignalcompression_amd.fastq` and
:mod:`~rawnanoporesignalcompression_amd.bam`, between whose steps they stand::

    bases = codec.collapse_codes(frame_codes, plan.read_frames, "ACGT")
    qual = quality.base_qual(codec, bases, frame_codes, frame_post, plan.read_frames)
    pats = (demux.barcode_patterns(front, barcodes, rear, max_dist=9) +
            demux.adapter_patterns(head=[adapter], tail=[demux.revcomp(adapter)], max_dist=4)).to(codec.device)
    hits = demux.find_patterns(codec, bases, pats, window=150)
    cls = demux.classify(codec, bases, hits, pats, nclasses=len(barcodes), min_sep=3)
    cut = demux.trim_reads(codec, bases, cls.lo, cls.hi, qual=qual, moves=(frame_codes, plan.read_frames, 5))
    for c in range(len(barcodes)):                                # no host wait up to here
        rec = bam.bam_records(codec, cut.decoded, cut.qual, ids, {"bc": cls.barcode}, keep=cls.barcode == c,
                              moves=(cut.codes, cut.read_frames, 5))

The project ships no kit sequences: the caller supplies them.  The host models (:func:`find_patterns_signal`,
:func:`classify_signal`, :func:`trim_reads_signal`) are those of :mod:`~rawnanoporesignalcompression_amd.host`.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .codec import DecodedReads, PGNanoCodec, _check, _ptr, _require_device
from .host import (DEMUX_NONE, PATTERN_NO_CLASS, _bam_moves, classify_signal, find_patterns_signal, trim_reads_signal)

__all__ = ["PatternSet", "barcode_patterns", "adapter_patterns", "revcomp", "find_patterns", "classify", "trim_reads",
           "barcode_tag", "PatternHits", "ReadClasses", "TrimmedReads", "find_patterns_signal", "classify_signal", "trim_reads_signal",
           "DEMUX_NONE", "PATTERN_NO_CLASS"]

_COMPLEMENT = bytes.maketrans(b"ACGTUNacgtun", b"TGCAANtgcaan")


def revcomp(seq) -> bytes:
    """The reverse complement of a sequence of ``ACGTUN`` in either case (``U`` gives ``A``); any other byte stays."""
    seq = seq.encode("ascii") if isinstance(seq, str) else bytes(seq)
    return seq.translate(_COMPLEMENT)[::-1]


def _seq_bytes(s) -> bytes:
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


class PatternSet:
    """Patterns for :func:`find_patterns` and :func:`classify`: their bytes, and per pattern the side (0 = head,
    1 = tail), the largest distance that is a hit and the class (a barcode's number, or :data:`PATTERN_NO_CLASS`
    for an adapter or primer).  ``max_dist`` and ``classes`` may be one value for all.  A length outside 1..128, a
    side other than 0 or 1 or a count outside 1..4,096 is a ``ValueError``.  Sets add up (``a + b``), and
    :meth:`to` uploads one once."""

    def __init__(self, patterns, sides, max_dist, classes=None):
        pats = [_seq_bytes(p) for p in patterns]
        n = len(pats)
        column = lambda v, default: [default] * n if v is None else ([int(v)] * n if np.ndim(v) == 0 else [int(x) for x in v])
        sides, max_dist, classes = column(sides, 0), column(max_dist, 0), column(classes, PATTERN_NO_CLASS)
        if not 1 <= n <= _native.PGN_DEMUX_MAX_PATTERNS:
            raise ValueError(f"a pattern set holds 1..{_native.PGN_DEMUX_MAX_PATTERNS} patterns (got {n})")
        if len(sides) != n or len(max_dist) != n or len(classes) != n:
            raise ValueError("sides, max_dist and classes hold one entry per pattern")
        for p, s in zip(pats, sides):
            if not 1 <= len(p) <= _native.PGN_DEMUX_MAX_PATTERN_BYTES:
                raise ValueError(f"a pattern has 1..{_native.PGN_DEMUX_MAX_PATTERN_BYTES} bytes (got {len(p)})")
            if s not in (0, 1):
                raise ValueError(f"a side is 0 (head) or 1 (tail) (got {s})")
        if any(not 0 <= v <= 0xFFFFFFFF for v in max_dist + classes):
            raise ValueError("max_dist and classes are uint32 values")
        self.patterns = pats
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(p) for p in pats])
        self._set(np.frombuffer(b"".join(pats), np.uint8), off, np.array(sides, np.uint8), np.array(max_dist, np.uint32),
                  np.array(classes, np.uint32))

    def _set(self, pat, pat_off, side, max_dist, pclass):
        self.pat, self.pat_off, self.side, self.max_dist, self.pclass = pat, pat_off, side, max_dist, pclass  # numpy
        self.device = None
        self.d_pat = self.d_pat_off = self.d_side = self.d_max_dist = self.d_pclass = None  # torch, after to()

    @classmethod
    def from_arrays(cls, pat, pat_off, side, max_dist, pclass):
        """A set of the arrays as the device reads them (uint8 bytes, uint32 offsets with one entry more than
        patterns, uint8 sides, uint32 distances and classes); nothing but their sizes is checked, and the device
        does not search a pattern with a bad side or length."""
        self = cls.__new__(cls)
        arrays = [np.array(np.asarray(a), dtype=t, order="C").reshape(-1) for a, t in
                  ((pat, np.uint8), (pat_off, np.uint32), (side, np.uint8), (max_dist, np.uint32), (pclass, np.uint32))]
        n = len(arrays[2])
        if not 1 <= n <= _native.PGN_DEMUX_MAX_PATTERNS or len(arrays[1]) != n + 1 or len(arrays[3]) != n or len(arrays[4]) != n:
            raise ValueError("pat_off holds one entry more than side, max_dist and pclass, which hold 1..4096")
        off = [int(v) for v in arrays[1]]
        self.patterns = [arrays[0][a:b].tobytes() if a <= b <= len(arrays[0]) else b"" for a, b in zip(off[:-1], off[1:])]
        self._set(*arrays)
        return self

    def __len__(self):
        return len(self.side)

    def __add__(self, other):
        if not isinstance(other, PatternSet):
            return NotImplemented
        return PatternSet.from_arrays(*(np.concatenate([x, y]) for x, y in (
            (self.pat, other.pat), (self.pat_off, other.pat_off[1:] + self.pat_off[-1]), (self.side, other.side),
            (self.max_dist, other.max_dist), (self.pclass, other.pclass))))

    def to(self, device):
        """The set with its arrays also on ``device`` (a device index or a torch device): one upload."""
        import torch

        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        out = PatternSet.from_arrays(self.pat, self.pat_off, self.side, self.max_dist, self.pclass)
        up = lambda a, view: torch.from_numpy(a.view(view)).to(dev)
        out.d_pat, out.d_pat_off, out.d_side = up(out.pat, np.uint8), up(out.pat_off, np.int32), up(out.side, np.uint8)
        out.d_max_dist, out.d_pclass = up(out.max_dist, np.int32), up(out.pclass, np.int32)
        out.device = dev
        return out


def barcode_patterns(front, barcodes, rear, *, max_dist, tail: bool = True) -> PatternSet:
    """For barcode ``c`` the head pattern ``front + barcodes[c] + rear`` of class ``c`` and, with ``tail``, its
    reverse complement as a tail pattern of the same class (what the far end of a read shows when both ends carry
    the barcode)."""
    front, rear = _seq_bytes(front), _seq_bytes(rear)
    pats, sides, classes = [], [], []
    for c, b in enumerate(barcodes):
        full = front + _seq_bytes(b) + rear
        pats.append(full)
        sides.append(0)
        classes.append(c)
        if tail:
            pats.append(revcomp(full))
            sides.append(1)
            classes.append(c)
    return PatternSet(pats, sides, max_dist, classes)


def adapter_patterns(head=(), tail=(), *, max_dist) -> PatternSet:
    """Patterns without a class: ``head`` at the reads' heads, ``tail`` at their tails, as they are written."""
    head, tail = list(head), list(tail)
    return PatternSet(head + tail, [0] * len(head) + [1] * len(tail), max_dist, None)


@dataclass
class PatternHits:
    """What :func:`find_patterns` leaves on the device: uint32 ``[reads, patterns]`` each (as int32 tensors)."""
    dist: "object"   # the least edit distance of the pattern in the read's window; 0xFFFFFFFF: not searched
    start: "object"  # where the best span starts, in bases from the read's start; 0xFFFFFFFF without a hit
    end: "object"    # where it ends (exclusive)


@dataclass
class ReadClasses:
    """What :func:`classify` leaves on the device: uint32 per read (as int32 tensors)."""
    barcode: "object"      # the read's class, or 0xFFFFFFFF (-1)
    best_dist: "object"    # the lowest distance of the best class, 0xFFFFFFFF without one
    second_dist: "object"  # of the second class
    lo: "object"           # the bases to keep are [lo, hi)
    hi: "object"


@dataclass
class TrimmedReads:
    """What :func:`trim_reads` leaves on the device."""
    decoded: DecodedReads   # the cut reads: seq, read_bases, status, and with moves base_frame and codes
    qual: "object"          # uint8 as decoded.seq, or None
    codes: "object"         # uint8: the kept frames' codes end to end, or None
    read_frames: "object"   # int64, reads + 1: the cut reads' frame offsets in codes, or None
    trim_frames: "object"   # int32 per read: the frames cut in front (times the stride: samples for ts), or None


def _decoded_reads(decoded, codec):
    """``(reads, capacity)`` of a decoded batch, checked as the record writers check it."""
    import torch

    n = int(decoded.status.numel())
    for name, t, size, dtype in (("read_bases", decoded.read_bases, n + 1, torch.int64), ("status", decoded.status, n, torch.int32)):
        _require_device(t, f"decoded.{name}", codec.device)
        if t.dtype != dtype or int(t.numel()) != size or not t.is_contiguous():
            raise ValueError(f"decoded.{name} must hold {size} contiguous {dtype} entries")
    _require_device(decoded.seq, "decoded.seq", codec.device)
    if decoded.seq.dtype != torch.uint8 or decoded.seq.dim() != 1 or not decoded.seq.is_contiguous():
        raise ValueError("decoded.seq must be a contiguous one-dimensional uint8 tensor")
    return n, int(decoded.seq.numel())


def _device_patterns(patterns, codec):
    if not isinstance(patterns, PatternSet) or patterns.device is None:
        raise ValueError("patterns must be a PatternSet on the device (PatternSet.to)")
    for name in ("d_pat", "d_pat_off", "d_side", "d_max_dist", "d_pclass"):
        _require_device(getattr(patterns, name), f"patterns.{name}", codec.device)
    return len(patterns)


def _u32_column(t, name, size, codec):
    _require_device(t, name, codec.device)
    if t.element_size() != 4 or t.is_floating_point() or int(t.numel()) != size or not t.is_contiguous():
        raise ValueError(f"{name} must hold {size} contiguous 32-bit integers")


def find_patterns(codec: PGNanoCodec, decoded: DecodedReads, patterns: PatternSet, window: int = 150,
                  stream: int | None = None) -> PatternHits:
    """Where each pattern fits best in each read's head or tail window (pgn_find_patterns_device):
    :func:`find_patterns_signal`, bit for bit.  decoded: the reads as :meth:`PGNanoCodec.collapse_codes` or
    :meth:`PGNanoCodec.ctc_decode` leaves them; patterns: a :class:`PatternSet` on the device; window: the bases
    searched at each end, 1..1,024.  No host wait."""
    import torch

    n, capacity = _decoded_reads(decoded, codec)
    P = _device_patterns(patterns, codec)
    window = int(window)
    if not 1 <= window <= _native.PGN_DEMUX_MAX_WINDOW:
        raise ValueError(f"window must lie in 1..{_native.PGN_DEMUX_MAX_WINDOW}")
    with codec._launch(stream) as ls:
        dist, start, end = (torch.empty((n, P), dtype=torch.int32, device=decoded.seq.device) for _ in range(3))
        nbytes = int(patterns.d_pat.numel())
        _check(codec._lib.pgn_find_patterns_device(
            codec._h, n, _ptr(decoded.seq) if capacity else 0, _ptr(decoded.read_bases), _ptr(decoded.status), capacity,
            window, P, _ptr(patterns.d_pat) if nbytes else 0, nbytes, _ptr(patterns.d_pat_off), _ptr(patterns.d_side),
            _ptr(patterns.d_max_dist), _ptr(dist) if n else 0, _ptr(start) if n else 0, _ptr(end) if n else 0,
            ls.cuda_stream))
    return PatternHits(dist, start, end)


def classify(codec: PGNanoCodec, decoded: DecodedReads, hits: PatternHits, patterns: PatternSet, nclasses: int,
             min_sep: int = 1, stream: int | None = None) -> ReadClasses:
    """The barcode of each read and the bases to keep (pgn_classify_reads_device): :func:`classify_signal`, bit for
    bit.  hits: what :func:`find_patterns` left for the same reads and patterns; nclasses: the number of barcodes;
    min_sep: how far the second class's distance must lie above the best's for the read to get the best class.
    ``keep = classes.barcode == c`` selects barcode ``c`` for the record writers, and ``classes.barcode`` is a tag
    column.  No host wait."""
    import torch

    n, capacity = _decoded_reads(decoded, codec)
    P = _device_patterns(patterns, codec)
    nclasses, min_sep = int(nclasses), int(min_sep)
    if not (0 <= nclasses <= 0xFFFFFFFF and 0 <= min_sep <= 0xFFFFFFFF):
        raise ValueError("nclasses and min_sep are uint32 values")
    for name in ("dist", "start", "end"):
        _u32_column(getattr(hits, name), f"hits.{name}", n * P, codec)
    with codec._launch(stream) as ls:
        out = [torch.empty(n, dtype=torch.int32, device=decoded.seq.device) for _ in range(5)]
        _check(codec._lib.pgn_classify_reads_device(
            codec._h, n, _ptr(decoded.read_bases), _ptr(decoded.status), capacity, P, _ptr(patterns.d_side),
            _ptr(patterns.d_max_dist), _ptr(patterns.d_pclass), nclasses, min_sep, *(_ptr(t) if n else 0 for t in
                                                                                (hits.dist, hits.start, hits.end)),
            *(_ptr(t) if n else 0 for t in out), ls.cuda_stream))
    return ReadClasses(*out)


def barcode_tag(barcode, names, unclassified=None):
    """The ``BC:Z`` / ``RG:Z`` column of a record call from :func:`classify`'s ``barcode``: read ``r`` gets
    ``names[barcode[r]]`` (a :func:`tags.zdict <rawnanoporesignalcompression_amd.tags.zdict>` column, the names
    uploaded once to the barcodes' device, or a :class:`tags.StringTable` that is there already).  A read without a
    class (:data:`DEMUX_NONE`, or any index at or above ``len(names)``) gets no tag; with ``unclassified="..."`` it
    gets that name, an extra entry that a ``torch.where`` on the device maps it to.  No host wait."""
    import torch

    from . import tags

    if isinstance(names, tags.StringTable):
        if unclassified is not None:
            raise ValueError("unclassified needs the names as a list: the extra entry joins their table")
        return tags.zdict(barcode, names.to(barcode.device))
    names = [_seq_bytes(s) for s in names]
    index = barcode
    if unclassified is not None:
        none = torch.full_like(barcode, len(names))
        index = torch.where((barcode < 0) | (barcode >= len(names)), none, barcode)   # uint32 bits: negative is above
        names = names + [_seq_bytes(unclassified)]
    return tags.zdict(index, tags.StringTable(names).to(barcode.device))


def trim_reads(codec: PGNanoCodec, decoded: DecodedReads, lo, hi, qual=None, moves=None, *, capacity=None,
               frame_capacity=None, stream: int | None = None) -> TrimmedReads:
    """Bases ``[lo, hi)`` of every read with everything it carries (pgn_trim_reads_device):
    :func:`trim_reads_signal`, bit for bit.  lo, hi: 32-bit integers per read, as :func:`classify` leaves them.
    qual: the phred characters, as ``decoded.seq``, or None.  moves: ``(codes, read_frames, stride)`` or ``(codes,
    read_frames, stride, frame_base)`` as for :func:`bam.bam_records <rawnanoporesignalcompression_amd.bam.bam_records>`
    (the stride is checked and not otherwise used); ``decoded`` must then carry ``base_frame``.  capacity,
    frame_capacity: the bases and frames the outputs hold (default: those of the inputs, which always suffice).
    ``TrimmedReads.decoded`` is what :func:`quality.base_qual`'s consumers and both record writers take; with moves
    give the writer ``(trimmed.codes, trimmed.read_frames, stride)``, and add ``trimmed.trim_frames * stride`` to a
    ``ts`` column.  No host wait."""
    import torch

    n, old_capacity = _decoded_reads(decoded, codec)
    _u32_column(lo, "lo", n, codec)
    _u32_column(hi, "hi", n, codec)
    if qual is not None:
        _require_device(qual, "qual", codec.device)
        if qual.dtype != torch.uint8 or qual.dim() != 1 or int(qual.numel()) != old_capacity or not qual.is_contiguous():
            raise ValueError(f"qual must be a contiguous uint8 tensor of {old_capacity} bytes, as decoded.seq")
    codes = read_frames = None
    frame_base = nframes = 0
    if moves is not None:
        codes, read_frames, _, frame_base = _bam_moves(moves)
        _require_device(codes, "moves[0]", codec.device)
        if codes.dtype != torch.uint8 or codes.dim() != 1 or not codes.is_contiguous():
            raise ValueError("moves[0], the frame codes, must be a contiguous one-dimensional uint8 tensor")
        _require_device(read_frames, "moves[1]", codec.device)
        if read_frames.dtype != torch.int64 or int(read_frames.numel()) != n + 1 or not read_frames.is_contiguous():
            raise ValueError(f"moves[1], the reads' frame offsets, must hold {n + 1} contiguous int64 entries")
        if decoded.base_frame is None:
            raise ValueError("with moves, decoded must carry base_frame (collapse_codes(..., base_frame=True))")
        _u32_column(decoded.base_frame, "decoded.base_frame", old_capacity, codec)
        nframes = int(codes.numel())
    capacity = old_capacity if capacity is None else int(capacity)
    frame_capacity = nframes if frame_capacity is None else int(frame_capacity)
    if capacity < 0 or frame_capacity < 0:
        raise ValueError("a capacity must not be negative")
    with codec._launch(stream) as ls:
        dev = decoded.seq.device
        seq = torch.empty(capacity, dtype=torch.uint8, device=dev)
        new_qual = torch.empty(capacity, dtype=torch.uint8, device=dev) if qual is not None else None
        bases = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        bf = new_codes = frames = cut = None
        if moves is not None:
            bf = torch.empty(capacity, dtype=torch.int32, device=dev)
            new_codes = torch.empty(frame_capacity, dtype=torch.uint8, device=dev)
            frames = torch.empty(n + 1, dtype=torch.int64, device=dev)
            cut = torch.empty(n, dtype=torch.int32, device=dev)
        _check(codec._lib.pgn_trim_reads_device(
            codec._h, n, _ptr(decoded.seq) if old_capacity else 0, _ptr(qual) if old_capacity else 0,
            _ptr(decoded.read_bases), _ptr(decoded.status) if n else 0, old_capacity, _ptr(lo) if n else 0,
            _ptr(hi) if n else 0, _ptr(decoded.base_frame) if moves is not None and old_capacity else 0, _ptr(read_frames),
            _ptr(codes) if nframes else 0, frame_base, nframes, _ptr(seq) if capacity else 0,
            _ptr(new_qual) if capacity else 0, _ptr(bf) if capacity else 0, capacity, _ptr(bases),
            _ptr(status) if n else 0, _ptr(new_codes) if frame_capacity else 0, frame_capacity, _ptr(frames),
            _ptr(cut) if n else 0, ls.cuda_stream))
    return TrimmedReads(DecodedReads(seq, bases, status, bf, None, new_codes, decoded.params), new_qual, new_codes, frames, cut)
