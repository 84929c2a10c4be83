"""Typed tags of the device record writers (include/pgnano_hip.h, "Typed record tags"): unsigned, signed and float
32-bit columns, and string columns from a dictionary or from a per-read pool, as wrappers that
:func:`bam.bam_records <rawnanoporesignalcompression_amd.bam.bam_records>` and :func:`fastq.fastq_records
<rawnanoporesignalcompression_amd.fastq.fastq_records>` take as values of ``tags``::

    qs = -10 * torch.log10(rq.err_sum.double() / n / 2**32)        # the caller's float
    rec = bam.bam_records(codec, bases, qual, ids,
        {"qs": tags.f32(qs.float()), "ch": ch, "ts": tags.i32(ts), "sm": tags.f32(centre), "sd": tags.f32(spread),
         "BC": demux.barcode_tag(cls.barcode, names), "pi": tags.zstr(parent_off, parent_bytes)},
        keep=rq.passed, moves=(codes, read_frames, 5), bgzf=False)

A dict whose values are all plain integer tensors still goes to the old calls, with at most 8 columns; one wrapper
among them sends the call to pgn_bam_records_tagged_device / pgn_fastq_records_tagged_device, with at most 16, and
a plain integer tensor is then a ``u32`` column.  The package's ``__all__`` and the methods of
:class:`~rawnanoporesignalcompression_amd.codec.PGNanoCodec` are a fixed surface, so the wrappers live here.  The
host models (:func:`tag_bytes_signal`, :func:`bam_records_tagged_signal`, :func:`fastq_records_tagged_signal`,
:func:`bam_bound_tagged`, :func:`fastq_bound_tagged`) are those of :mod:`~rawnanoporesignalcompression_amd.host`.
"""
from __future__ import annotations

import numpy as np

from . import _native
from .host import (REC_MAX_TAGS, TAG_DICT, TAG_F32, TAG_I32, TAG_MAX_STRING, TAG_STR, TAG_U32, TagColumn,
                   bam_bound_tagged, bam_records_tagged_signal, fastq_bound_tagged, fastq_records_tagged_signal,
                   tag_bytes_signal)

__all__ = ["u32", "i32", "f32", "zdict", "zstr", "Tag", "StringTable", "TagColumn", "tag_bytes_signal",
           "bam_records_tagged_signal", "fastq_records_tagged_signal", "bam_bound_tagged", "fastq_bound_tagged",
           "TAG_U32", "TAG_I32", "TAG_F32", "TAG_DICT", "TAG_STR", "REC_MAX_TAGS", "TAG_MAX_STRING"]


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr")


class StringTable:
    """Strings end to end with their offsets: ``off`` (uint32, one entry more than strings) and ``data`` (uint8).
    Built from a list of ``bytes`` or ``str`` (each printable ASCII, at most 255 bytes, else a ``ValueError``) or,
    with :meth:`from_arrays`, from the arrays as the device reads them, unchecked: the device refuses per read what
    an offset or a byte makes invalid.  :meth:`to` uploads a table once."""

    def __init__(self, strings):
        items = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strings]
        for s in items:
            if len(s) > TAG_MAX_STRING or any(ch < 0x20 or ch > 0x7E for ch in s):
                raise ValueError(f"a tag string holds at most {TAG_MAX_STRING} bytes in 0x20..0x7E (got {s[:40]!r})")
        off = np.zeros(len(items) + 1, np.uint32)
        off[1:] = np.cumsum([len(s) for s in items])
        self._set(off, np.frombuffer(b"".join(items), np.uint8).copy())

    def _set(self, off, data):
        self.off, self.data = off, data          # numpy, or None for a table made of device tensors
        self.device = None
        self.d_off = self.d_data = None          # torch, after to()

    @classmethod
    def from_arrays(cls, off, data):
        """A table of the arrays themselves: numpy arrays (or lists), or torch tensors already on a device (32-bit
        integer offsets and uint8 bytes, contiguous)."""
        self = cls.__new__(cls)
        if _is_tensor(off) or _is_tensor(data):
            if not (_is_tensor(off) and _is_tensor(data)) or off.device != data.device:
                raise ValueError("offsets and bytes must both be tensors on one device, or both host arrays")
            if off.element_size() != 4 or off.is_floating_point() or off.dim() != 1 or not off.is_contiguous():
                raise ValueError("the offsets must be a contiguous one-dimensional tensor of 32-bit integers")
            if data.element_size() != 1 or data.dim() != 1 or not data.is_contiguous():
                raise ValueError("the bytes must be a contiguous one-dimensional uint8 tensor")
            self._set(None, None)
            self.d_off, self.d_data, self.device = off, data, off.device
            return self
        self._set(np.array(np.asarray(off), dtype=np.uint32, order="C").reshape(-1),
                  np.array(np.asarray(data), dtype=np.uint8, order="C").reshape(-1))
        return self

    def __len__(self):
        return int((self.off if self.off is not None else self.d_off).shape[0]) - 1

    @property
    def nbytes(self) -> int:
        return int((self.data if self.data is not None else self.d_data).shape[0])

    def to(self, device):
        """The table with its arrays also on ``device`` (a device index or a torch device): one upload."""
        import torch

        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device is not None and self.device == dev:
            return self
        if self.off is None:
            out = StringTable.from_arrays(self.d_off.to(dev), self.d_data.to(dev))
            return out
        out = StringTable.from_arrays(self.off, self.data)
        out.d_off = torch.from_numpy(out.off.view(np.int32)).to(dev)
        out.d_data = torch.from_numpy(out.data).to(dev)
        out.device = dev
        return out


class Tag:
    """A typed column: its ``type`` (``TAG_*``), its ``values`` (one 32-bit entry per read, None for ``zstr``) and
    for the string types its :class:`StringTable`.  ``column`` is the same as a :class:`TagColumn` for the host
    models."""

    def __init__(self, type, values=None, table=None):
        self.type, self.values, self.table = int(type), values, table

    def to(self, device):
        """The column with its string table (and host values) on ``device``."""
        import torch

        values = self.values
        if values is not None and not _is_tensor(values):
            dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
            values = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
        return Tag(self.type, values, None if self.table is None else self.table.to(device))

    @property
    def column(self) -> TagColumn:
        t = self.table
        if t is None:
            return TagColumn(self.type, self.values)
        off, data = (t.off, t.data) if t.off is not None else (t.d_off, t.d_data)
        return TagColumn(self.type, self.values, off, data, len(t) if self.type == TAG_DICT else 0, t.nbytes)


def _values(t, kinds, what):
    if _is_tensor(t):
        ok = t.element_size() == 4 and t.is_floating_point() == (kinds == "f")
    else:
        t = np.ascontiguousarray(t)
        ok = t.dtype.itemsize == 4 and t.dtype.kind in kinds
    if not ok:
        raise ValueError(f"{what} takes 32-bit {'floats' if kinds == 'f' else 'integers'}, one per read")
    return t


def u32(t) -> Tag:
    """``XX:I:`` in BAM, ``XX:i:dec`` in FASTQ: the 32 bits of an integer tensor read as unsigned, as a plain
    tensor in ``tags`` is."""
    return Tag(TAG_U32, _values(t, "iu", "u32"))


def i32(t) -> Tag:
    """``XX:i:`` in BAM, ``XX:i:[-]dec`` in FASTQ: the 32 bits read as signed."""
    return Tag(TAG_I32, _values(t, "iu", "i32"))


def f32(t) -> Tag:
    """``XX:f:`` in BAM, the four bytes as stored; FASTQ records refuse it."""
    return Tag(TAG_F32, _values(t, "f", "f32"))


def zdict(index, strings) -> Tag:
    """``XX:Z:strings[index[r]]``: a 32-bit index per read into ``strings`` (a list of ``bytes`` or ``str``, or a
    :class:`StringTable`); an index at or above ``len(strings)`` leaves the read without the tag."""
    table = strings if isinstance(strings, StringTable) else StringTable(strings)
    return Tag(TAG_DICT, _values(index, "iu", "zdict's index"), table)


def zstr(offsets, data=None) -> Tag:
    """``XX:Z:`` with a string per read: ``zstr(list_of_bytes)``, or ``zstr(offsets, data)`` with reads + 1 32-bit
    offsets into the bytes of ``data`` (host arrays, or tensors on the device)."""
    if data is None:
        table = offsets if isinstance(offsets, StringTable) else StringTable(offsets)
    else:
        table = StringTable.from_arrays(offsets, data)
    return Tag(TAG_STR, None, table)


def has_typed(tags) -> bool:
    """Whether a record call's ``tags`` hold a wrapper of this module (the call is then the tagged one)."""
    return any(isinstance(v, Tag) for v in (tags or {}).values())


def native_columns(codec, tags, nreads, text: bool):
    """``(pgn_record_tags, the wrappers in order)`` of a record call's ``tags``, checked; a plain integer tensor is
    a ``u32`` column."""
    from .codec import _ptr, _require_device
    from .host import _fastq_tags

    items = [(name, v if isinstance(v, Tag) else None, v) for name, v in (tags or {}).items()]
    if len(items) > REC_MAX_TAGS:
        raise ValueError(f"at most {REC_MAX_TAGS} typed tags")
    out = _native.RecordTags(len(items), 0)
    cols = []
    for k, (name, tag, plain) in enumerate(items):
        if tag is None:
            if not _is_tensor(plain) or plain.is_floating_point():
                raise ValueError(f"tags[{name!r}] must hold {nreads} contiguous 32-bit integers (a float column is tags.f32)")
            tag = u32(plain)
        if tag.type == TAG_F32 and text:
            raise ValueError(f"tags[{name!r}]: a float tag has no text rule, FASTQ records take no f32 column")
        _fastq_tags([(name, ())], 0)                         # the name
        c = out.col[k]
        c.name[:] = list(name.encode("ascii"))
        c.type = tag.type
        if tag.type != TAG_STR:
            t = tag.values
            if not _is_tensor(t):
                raise ValueError(f"tags[{name!r}]: the values must be a device tensor (Tag.to)")
            _require_device(t, f"tags[{name!r}]", codec.device)
            if t.element_size() != 4 or int(t.numel()) != nreads or not t.is_contiguous():
                raise ValueError(f"tags[{name!r}] must hold {nreads} contiguous 32-bit values")
            c.d_values = _ptr(t) if nreads else 0
        if tag.table is not None:
            tb = tag.table
            if tb.device is None:
                raise ValueError(f"tags[{name!r}]: the string table must be on the device (Tag.to or StringTable.to)")
            _require_device(tb.d_off, f"tags[{name!r}] offsets", codec.device)
            _require_device(tb.d_data, f"tags[{name!r}] bytes", codec.device)
            if tag.type == TAG_STR and len(tb) != nreads:
                raise ValueError(f"tags[{name!r}] must hold {nreads + 1} offsets, a string per read")
            c.nstrings = len(tb) if tag.type == TAG_DICT else 0
            c.d_str_off = _ptr(tb.d_off)
            c.d_strings = _ptr(tb.d_data) if tb.nbytes else 0
            c.str_capacity = tb.nbytes
        cols.append(tag)
    return out, cols
