"""Batched checksums on the GPU (device-resident and host-resident), over the C ABI.

The reference has no batch API: every packet's checksum is one
util::compute_ones_comp call on the thread handling it.  A batch
here is a packet ARENA (one uint8 buffer) plus per-packet descriptors:

* ``off``  — int64 byte offset of each packet in the arena (any alignment);
* ``length`` — int32 length in bytes;
* ``seed`` — optional 16-bit seed per packet (the pseudo-header sum callers
  pass as in_checksum / initial_sum: tcp.rs:845-848, udp.rs:158-168, icmp.rs:63-71);
* ``complement`` — store ``0xffff ^ sum`` (what every call site stores or tests).

PyTorch only provides device memory and the stream; the compute is the
hand-written gfx950 kernel in csrc/rns_checksum.hip.  There is no CPU fallback:
a missing library or device raises.

Every wrapper checks its tensors before the call: dtype and contiguity (TypeError /
ValueError), one size per descriptor form, and that every descriptor, seed, field and
output tensor is on the arena's device (ValueError) — a pointer of another device must
never reach a kernel.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def _require_cuda(t: torch.Tensor, name: str, dtypes) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on a GPU device (got {t.device}); there is no CPU fallback")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} dtype {t.dtype} not in {dtypes}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_U16 = (torch.uint16, torch.int16)
_U8 = (torch.uint8,)
_I32 = (torch.int32,)
_I64 = (torch.int64,)


def _descriptors(arena: torch.Tensor, *desc) -> torch.device:
    """The arena and its descriptor tensors ``(name, tensor, dtypes)``: GPU tensors of the
    right dtype, contiguous, all on the arena's device (which is returned)."""
    _require_cuda(arena, "arena", _U8)
    for name, t, dtypes in desc:
        _require_cuda(t, name, dtypes)
    for name, t, _ in desc:
        if t.device != arena.device:
            raise ValueError(f"{name} is on {t.device}, the arena on {arena.device}")
    return arena.device


def _per_packet(t: torch.Tensor | None, name: str, n: int, dev: torch.device, dtypes=_U16) -> int | None:
    """Pointer of an optional per-packet tensor (seed / field / out / l4_sum: 16-bit; status:
    uint8) of exactly n entries on the arena's device, or None."""
    if t is None:
        return None
    _require_cuda(t, name, dtypes)
    if t.numel() != n or t.device != dev:
        raise ValueError(f"{name} must have one entry per packet ({n}) on {dev}")
    return t.data_ptr()


def _out(out: torch.Tensor | None, n: int, dev: torch.device) -> torch.Tensor:
    """The checksum output: the caller's (checked like any per-packet tensor) or a new one."""
    if out is None:
        return torch.empty(n, dtype=torch.uint16, device=dev)
    _per_packet(out, "out", n, dev)
    return out


def _status(status: torch.Tensor | None, n: int, dev: torch.device) -> torch.Tensor:
    """The uint8 status output: the kernel writes n entries, so an undersized or misplaced
    buffer is refused."""
    if status is None:
        return torch.empty(n, dtype=torch.uint8, device=dev)
    _per_packet(status, "status", n, dev, _U8)
    return status


def _explicit(arena, off, length, off_dtypes=_I64) -> tuple[int, torch.device]:
    """Explicit descriptors (off, length): (n, device)."""
    dev = _descriptors(arena, ("off", off, off_dtypes), ("length", length, _I32))
    n = off.numel()
    if length.numel() != n:
        raise ValueError("off and length must have the same number of packets")
    if n >= 2 ** 32:
        raise ValueError("at most 2^32-1 packets per call")
    return n, dev


def _packed(arena, blk_off, len16, align_log2, align_range, exact: bool = False) -> tuple[int, torch.device]:
    """Packed descriptors (one offset per 64 packets, u16 lengths): (n, device).  ``exact``:
    exactly ceil(n/64) block offsets, else at least that many.  ``align_range``: the wrapper's
    (lowest, highest) align_log2, or None where the C ABI alone checks it."""
    dev = _descriptors(arena, ("blk_off", blk_off, _I64), ("len16", len16, _U16))
    n = len16.numel()
    need = (n + 63) // 64
    if blk_off.numel() != need if exact else blk_off.numel() < need:
        raise ValueError("blk_off must have one entry per 64 packets")
    if align_range is not None and not align_range[0] <= align_log2 <= align_range[1]:
        raise ValueError(f"align_log2 must be in {align_range[0]}..{align_range[1]}")
    if n >= 2 ** 32:
        raise ValueError("at most 2^32-1 packets per call")
    return n, dev


def _chain(arena, frag_off, frag_len, first) -> tuple[int, int, torch.device]:
    """Chain descriptors (CSR: packet i = fragments first[i] .. first[i+1]): (n, n_frags, device)."""
    dev = _descriptors(arena, ("frag_off", frag_off, _I64), ("frag_len", frag_len, _I32), ("first", first, _I32))
    nf = frag_off.numel()
    n = first.numel() - 1
    if frag_len.numel() != nf or n < 0:
        raise ValueError("frag_off/frag_len sizes differ or first is empty")
    if n > _lib.RNS_CHAIN_MAX_PACKETS or nf >= 2 ** 32:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} packets and 2^32-1 fragments per chain call")
    return n, nf, dev


def _local_addrs(local_ipv4, local_ipv6) -> tuple[bytes, bytes]:
    if len(local_ipv4) != 4 or len(local_ipv6) != 16:
        raise ValueError("local_ipv4 must be 4 bytes and local_ipv6 16 bytes")
    return bytes(local_ipv4), bytes(local_ipv6)


def _bad_ptr(bad: torch.Tensor | None, dev: torch.device):
    """The rejected-descriptor counter the kernels atomically add to: an int32 tensor of at
    least one entry on the arena's device, or None."""
    if bad is None:
        return None
    _require_cuda(bad, "bad", _I32)
    if bad.numel() < 1 or bad.device != dev:
        raise ValueError(f"bad must be an int32 counter (at least 1 entry) on {dev}")
    return bad.data_ptr()


def _flags(complement: bool, runs: bool = False, tx_packed: bool = False) -> int:
    return (_lib.RNS_FLAG_COMPLEMENT if complement else 0) | (_lib.RNS_FLAG_CHAIN_RUNS if runs else 0) | \
        (_lib.RNS_FLAG_CHAIN_TX_PACKED if tx_packed else 0)


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _call(name: str, dev: torch.device, *args) -> None:
    """One C ABI call on the arena's device and its current stream (the last argument)."""
    with torch.cuda.device(dev):
        st = getattr(_lib.load(), name)(*args, _stream_handle(dev))
    _lib.check(st, name)


def _ptr(t: torch.Tensor | None):
    """A tensor's address; None (a null pointer) for no tensor and for an empty one (place, flow, send, icmp, udp)."""
    return t.data_ptr() if t is not None and t.numel() else None


def _nonnull(dev: torch.device):
    """``ptr(t)`` for an entry point that wants a pointer even where nothing is read: an empty tensor's (its
    data_ptr is null) is the address of 16 bytes that live as long as ``ptr``."""
    keep = torch.empty(16, dtype=torch.uint8, device=dev)
    return lambda t: t.data_ptr() or keep.data_ptr()


def _bytes_of(t: torch.Tensor, name: str, n: int, item: int, dev) -> None:
    _require_cuda(t, name, _U8)
    if t.numel() != n * item or (dev is not None and t.device != dev):
        raise ValueError(f"{name} must hold {n} records of {item} bytes on the meta's device")


def _work_bytes(name: str, *args) -> int:
    """A workspace size query of the C ABI (``rns_..._work``): its last argument is the u64 result."""
    need = ctypes.c_uint64(0)
    _lib.check(getattr(_lib.load(), name)(*args, ctypes.byref(need)), name)
    return int(need.value)


def _workspace(work: torch.Tensor | None, need: int, dev, dtype=torch.uint8, complaint: str | None = None) -> torch.Tensor:
    """The caller's workspace (``dtype`` uint8 or int64) checked for ``need`` bytes, 8-byte aligned, or a new one."""
    item = 8 if dtype == torch.int64 else 1
    if work is None:
        return torch.empty(-(-max(need, 8) // item), dtype=dtype, device=dev)
    _require_cuda(work, "work", (dtype,))
    if work.numel() * item < need or work.device != dev or work.data_ptr() & 7:
        raise ValueError(complaint or f"work must hold {need} bytes, 8-byte aligned, on the meta's device")
    return work


def _seq_gt(a: int, b: int) -> bool:
    """util.rs:155-158."""
    d = (a - b) & 0xFFFFFFFF
    return d < 0x80000000 and d != 0


class _BoundBatch:
    """A batch bound to one C ABI entry point: the subclass's constructor validates and
    marshals (``_bind``), so each launch is a single ctypes call with pre-marshalled
    arguments.  Launches go to the stream that was current at construction."""

    def _bind(self, name: str, args: tuple, keep: tuple, out: torch.Tensor, n: int, dev: torch.device) -> None:
        self._name, self._fn, self._args = name, getattr(_lib.load(), name), args + (_stream_handle(dev),)
        self._keep = keep  # keep the tensors alive as long as the bound pointers
        self.out, self.n, self.device = out, n, dev

    def __call__(self) -> torch.Tensor:
        if self.n:
            # The bound stream handle belongs to self.device (the null stream is 0): launch
            # with that device current even if the caller has switched devices since.
            if torch.cuda.current_device() != self.device.index:
                with torch.cuda.device(self.device):
                    st = self._fn(*self._args)
            else:
                st = self._fn(*self._args)
            if st != _lib.RNS_OK:
                raise _lib.ChecksumError(st, self._name)
        return self.out


class PreparedBatch(_BoundBatch):
    """A device-resident batch bound to the C ABI once: validation and argument
    marshalling happen here, so each launch is a single ctypes call (a few µs of
    host time).  Launches go to the stream that was current at construction.

    ``shape`` = (variant, lanes_per_packet, unroll, max_blocks) overrides the
    automatic kernel shape (tuning); see rns_csum_batch_dev_cfg.

    ``compact=True`` selects the compact descriptor form explicitly
    (rns_csum_batch_dev_off32): ``off`` is then an int32 tensor whose bits are
    UNSIGNED 32-bit offsets (arenas below 4 GiB; 10 B of descriptors per packet
    instead of 14).  Otherwise ``off`` must be int64; an int32 ``off`` without
    ``compact=True`` is a TypeError, never a silent switch of the descriptor form.
    """

    def __init__(self, arena: torch.Tensor, off: torch.Tensor, length: torch.Tensor,
                 seed: torch.Tensor | None = None, *, complement: bool = False, out: torch.Tensor | None = None,
                 len_hint: int = 0, bad: torch.Tensor | None = None,
                 shape: tuple[int, int, int, int] | None = None, compact: bool = False):
        n, dev = _explicit(arena, off, length, _I32 if compact else _I64)
        if compact and shape is not None:
            raise ValueError("shape overrides take 64-bit offsets")
        seed_ptr = _per_packet(seed, "seed", n, dev)
        out = _out(out, n, dev)
        head = (arena.data_ptr(), arena.numel(), off.data_ptr(), length.data_ptr(), seed_ptr, out.data_ptr(), n,
                _flags(complement))
        keep = (arena, off, length, seed, out, bad)
        if shape is None:
            self._bind("rns_csum_batch_dev_off32" if compact else "rns_csum_batch_dev",
                       head + (int(len_hint), _bad_ptr(bad, dev)), keep, out, n, dev)
        else:
            var, g, u, mb = shape
            self._bind("rns_csum_batch_dev_cfg", head + (var, g, u, mb, _bad_ptr(bad, dev)), keep, out, n, dev)


def packed_layout(length, align_log2: int = 4, first_off: int = 0):
    """Offsets of the packed form (rns_packed_layout): packets back to back in index
    order, each starting at the next multiple of 2**align_log2.  ``length``: lengths
    (< 65536).  Returns (blk_off uint64 [ceil(n/64)], off uint64 [n], end)."""
    ln = np.asarray(length)
    if ln.size and (int(ln.max()) > 0xFFFF or int(ln.min()) < 0):
        raise ValueError("packed descriptors hold u16 lengths (< 65536)")
    len16 = np.ascontiguousarray(ln, dtype=np.uint16)
    n = int(len16.size)
    blk = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    off = np.zeros(max(n, 1), dtype=np.uint64)
    end = ctypes.c_uint64(0)
    st = _lib.load().rns_packed_layout(len16.ctypes.data, n, int(align_log2), int(first_off), blk.ctypes.data,
                                       off.ctypes.data, ctypes.byref(end))
    _lib.check(st, "rns_packed_layout")
    return blk[:(n + 63) // 64], off[:n], int(end.value)


class PackedBatch(_BoundBatch):
    """A device-resident batch in the packed form (rns_csum_batch_packed_dev), bound
    once like PreparedBatch: ``blk_off`` int64 [ceil(n/64)] (the offset of every 64th
    packet), ``len16`` int16/uint16 [n] (lengths as unsigned 16-bit), packets back to
    back at 2**align_log2 boundaries (see packed_layout)."""

    def __init__(self, arena: torch.Tensor, blk_off: torch.Tensor, len16: torch.Tensor,
                 seed: torch.Tensor | None = None, *, align_log2: int = 4, complement: bool = False,
                 out: torch.Tensor | None = None, len_hint: int = 0, bad: torch.Tensor | None = None):
        n, dev = _packed(arena, blk_off, len16, align_log2, (0, 12), exact=True)
        seed_ptr = _per_packet(seed, "seed", n, dev)
        out = _out(out, n, dev)
        self._bind("rns_csum_batch_packed_dev",
                   (arena.data_ptr(), arena.numel(), blk_off.data_ptr(), len16.data_ptr(), int(align_log2), seed_ptr,
                    out.data_ptr(), n, _flags(complement), int(len_hint), _bad_ptr(bad, dev)),
                   (arena, blk_off, len16, seed, out, bad), out, n, dev)


def csum_batch_packed(arena: torch.Tensor, blk_off: torch.Tensor, len16: torch.Tensor,
                      seed: torch.Tensor | None = None, *, align_log2: int = 4, complement: bool = False,
                      out: torch.Tensor | None = None, len_hint: int = 0,
                      bad: torch.Tensor | None = None) -> torch.Tensor:
    """Checksum a batch in the packed form (offsets implied by lengths; see PackedBatch)."""
    _require_cuda(arena, "arena", _U8)
    with torch.cuda.device(arena.device):
        return PackedBatch(arena, blk_off, len16, seed, align_log2=align_log2, complement=complement, out=out,
                           len_hint=len_hint, bad=bad)()


def csum_batch(arena: torch.Tensor, off: torch.Tensor, length: torch.Tensor, seed: torch.Tensor | None = None,
               *, complement: bool = False, out: torch.Tensor | None = None, len_hint: int = 0,
               bad: torch.Tensor | None = None, shape: tuple[int, int, int, int] | None = None,
               compact: bool = False) -> torch.Tensor:
    """Checksum every packet of a device-resident batch; returns uint16 [n] on the same device.

    Launches on the current torch stream of ``arena``'s device and returns
    without synchronising.  A packet outside the arena yields 0 and increments
    ``bad`` (int32 [1] device tensor) if given.  ``shape`` = (variant,
    lanes_per_packet, unroll, max_blocks) overrides the kernel shape (tuning).
    ``compact=True``: ``off`` holds unsigned 32-bit offsets in an int32 tensor.
    """
    _require_cuda(arena, "arena", _U8)
    with torch.cuda.device(arena.device):
        return PreparedBatch(arena, off, length, seed, complement=complement, out=out, len_hint=len_hint, bad=bad,
                             shape=shape, compact=compact)()


class StridedBatch(_BoundBatch):
    """A device-resident batch of equal-length packets at a fixed stride
    (rns_csum_batch_strided_dev), bound once like PreparedBatch: packet i =
    arena[first_off + i*stride : + length].  No offset or length descriptors travel."""

    def __init__(self, arena: torch.Tensor, n: int, stride: int, length: int, *, first_off: int = 0,
                 seed: torch.Tensor | None = None, complement: bool = False,
                 out: torch.Tensor | None = None, bad: torch.Tensor | None = None):
        dev = _descriptors(arena)
        if n < 0 or n >= 2 ** 32 or stride < 0 or not 0 <= length < 2 ** 32 or first_off < 0:
            raise ValueError("n, stride, length and first_off must be non-negative (n, length < 2^32)")
        n = int(n)
        seed_ptr = _per_packet(seed, "seed", n, dev)
        out = _out(out, n, dev)
        self._bind("rns_csum_batch_strided_dev",
                   (arena.data_ptr(), arena.numel(), int(first_off), int(stride), int(length), seed_ptr,
                    out.data_ptr(), n, _flags(complement), _bad_ptr(bad, dev)),
                   (arena, seed, out, bad), out, n, dev)


def csum_batch_strided(arena: torch.Tensor, n: int, stride: int, length: int, *, first_off: int = 0,
                       seed: torch.Tensor | None = None, complement: bool = False,
                       out: torch.Tensor | None = None, bad: torch.Tensor | None = None) -> torch.Tensor:
    """Packets at a fixed stride: packet i = arena[first_off + i*stride : + length]."""
    _require_cuda(arena, "arena", _U8)
    with torch.cuda.device(arena.device):
        return StridedBatch(arena, n, stride, length, first_off=first_off, seed=seed, complement=complement,
                            out=out, bad=bad)()


def csum_chain(arena: torch.Tensor, frag_off: torch.Tensor, frag_len: torch.Tensor, first: torch.Tensor,
               seed: torch.Tensor | None = None, *, complement: bool = False, out: torch.Tensor | None = None,
               frag_sums: torch.Tensor | None = None, bad: torch.Tensor | None = None,
               frag_len_hint: int = 512, runs: bool = False, tx_packed: bool = False) -> torch.Tensor:
    """util.rs:112 ``compute_buffer_ones_comp`` for a batch of fragment chains.

    Packet i = fragments ``first[i] .. first[i+1]`` (``first``: int32 [n+1]) of
    ``(frag_off, frag_len)``; each fragment is folded on its own like the reference,
    in one pass (``frag_sums`` is accepted for compatibility and unused).
    ``runs``: RNS_FLAG_CHAIN_RUNS, the hint that fragments are often back-to-back
    views of one buffer (same results either way).  ``tx_packed``: RNS_FLAG_CHAIN_TX_PACKED
    (see csum_chain_fill).
    """
    n, nf, dev = _chain(arena, frag_off, frag_len, first)
    seed_ptr = _per_packet(seed, "seed", n, dev)
    out = _out(out, n, dev)
    _call("rns_csum_chain_dev", dev, arena.data_ptr(), arena.numel(), frag_off.data_ptr(), frag_len.data_ptr(), nf,
          first.data_ptr(), seed_ptr, out.data_ptr(), n, _flags(complement, runs, tx_packed), int(frag_len_hint),
          frag_sums.data_ptr() if frag_sums is not None else None, _bad_ptr(bad, dev))
    return out


def _fill_ptrs(seed, field, field_off, out, n: int, dev: torch.device, max_field_off: int | None = None):
    """The fills' optional per-packet tensors: (seed, field, out) pointers; ``max_field_off``
    bounds a ``field_off`` that applies to every packet."""
    ptrs = tuple(_per_packet(t, name, n, dev) for name, t in (("seed", seed), ("field", field), ("out", out)))
    if max_field_off is not None and field is None and not 0 <= int(field_off) <= max_field_off:
        raise ValueError(f"field_off must be in 0..{max_field_off}")
    return ptrs


def csum_chain_fill(arena: torch.Tensor, frag_off: torch.Tensor, frag_len: torch.Tensor, first: torch.Tensor,
                    seed: torch.Tensor | None = None, *, field: torch.Tensor | None = None, field_off: int = 16,
                    complement: bool = True, out: torch.Tensor | None = None, bad: torch.Tensor | None = None,
                    frag_len_hint: int = 512, runs: bool = False, tx_packed: bool = False) -> torch.Tensor | None:
    """Transmit fill over fragment chains (rns_csum_chain_fill_dev): packet i = fragments
    ``first[i] .. first[i+1]`` as for ``csum_chain``; its checksum field is at byte
    ``field[i]`` (or ``field_off``) of its FIRST fragment (the head fragment
    alloc_header prepended, buf.rs:262-291), counts as zero, and receives
    ``compute_buffer_ones_comp(seed, chain) ^ 0xffff`` big-endian (tcp.rs:957-973).
    ``tx_packed``: RNS_FLAG_CHAIN_TX_PACKED, the hint that packets are [head <= 4 chunks,
    payload run] with the payloads packed at 16-byte starts (same results either way).
    Returns ``out`` if given."""
    n, nf, dev = _chain(arena, frag_off, frag_len, first)
    seed_ptr, field_ptr, out_ptr = _fill_ptrs(seed, field, field_off, out, n, dev, max_field_off=2 ** 32 - 1)
    _call("rns_csum_chain_fill_dev", dev, arena.data_ptr(), arena.numel(), frag_off.data_ptr(), frag_len.data_ptr(),
          nf, first.data_ptr(), seed_ptr, field_ptr, int(field_off), out_ptr, n, _flags(complement, runs, tx_packed),
          int(frag_len_hint), _bad_ptr(bad, dev))
    return out


def csum_fill(arena: torch.Tensor, off: torch.Tensor, length: torch.Tensor, seed: torch.Tensor | None = None, *,
              field: torch.Tensor | None = None, field_off: int = 16, complement: bool = True,
              out: torch.Tensor | None = None, bad: torch.Tensor | None = None) -> torch.Tensor | None:
    """Transmit in-place fill: each packet's checksum, computed with its 2-byte field
    counted as zero, is stored big-endian into the field (tcp.rs:970-973 ``set_be16``).

    ``field`` (int16/uint16 [n]) gives per-packet field offsets, else ``field_off``
    for all (TCP 16, UDP 6, ICMP 2, IPv4 header 10).  Returns ``out`` if given.
    """
    n, dev = _explicit(arena, off, length)
    seed_ptr, field_ptr, out_ptr = _fill_ptrs(seed, field, field_off, out, n, dev)
    _call("rns_csum_fill_dev", dev, arena.data_ptr(), arena.numel(), off.data_ptr(), length.data_ptr(), seed_ptr,
          field_ptr, int(field_off), out_ptr, n, _flags(complement), _bad_ptr(bad, dev))
    return out


def csum_fill_packed(arena: torch.Tensor, blk_off: torch.Tensor, len16: torch.Tensor,
                     seed: torch.Tensor | None = None, *, align_log2: int = 4, field: torch.Tensor | None = None,
                     field_off: int = 16, complement: bool = True, out: torch.Tensor | None = None,
                     len_hint: int = 0, bad: torch.Tensor | None = None) -> torch.Tensor | None:
    """Transmit in-place fill of a packed arena (rns_csum_fill_packed_dev): ``csum_fill``'s
    result and stores, with the packed form's descriptors (see PackedBatch; align_log2 >= 4)."""
    n, dev = _packed(arena, blk_off, len16, align_log2, (4, 12), exact=True)
    # packed lengths are u16: no packet can hold a field past byte 65533 (the C ABI itself
    # rejects every packet of such a call and leaves the arena unchanged)
    seed_ptr, field_ptr, out_ptr = _fill_ptrs(seed, field, field_off, out, n, dev, max_field_off=0xFFFD)
    _call("rns_csum_fill_packed_dev", dev, arena.data_ptr(), arena.numel(), blk_off.data_ptr(), len16.data_ptr(),
          int(align_log2), seed_ptr, field_ptr, int(field_off), out_ptr, n, _flags(complement), int(len_hint),
          _bad_ptr(bad, dev))
    return out


def rx_verify(arena: torch.Tensor, off: torch.Tensor, length: torch.Tensor, local_ipv4: bytes, local_ipv6: bytes,
              *, status: torch.Tensor | None = None, l4_sum: torch.Tensor | None = None) -> torch.Tensor:
    """Receive verify of a batch of IP datagrams (rns_rx_verify_dev): returns a uint8
    status per packet (RNS_RX_* bits; RNS_RX_ACCEPT = the stack would deliver it)."""
    n, dev = _explicit(arena, off, length)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    _call("rns_rx_verify_dev", dev, arena.data_ptr(), arena.numel(), off.data_ptr(), length.data_ptr(), n, ip4, ip6,
          status.data_ptr(), _per_packet(l4_sum, "l4_sum", n, dev))
    return status


def rx_verify_chain(arena: torch.Tensor, frag_off: torch.Tensor, frag_len: torch.Tensor, first: torch.Tensor,
                    local_ipv4: bytes, local_ipv6: bytes, *, status: torch.Tensor | None = None,
                    l4_sum: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Receive verify of NetBuffer fragment chains (rns_rx_verify_chain_dev): datagram i =
    fragments ``first[i] .. first[i+1]`` (``first``: int32 [n+1]) of ``(frag_off, frag_len)``,
    the chains of csum_chain, decided as the reference decides on a NetBuffer (header() = the
    first fragment, trim_head, the L4 sum folded fragment by fragment).  Nothing is written to
    the arena.  Returns ``(status, l4_sum)``: uint8 RNS_RX_* bits per datagram, and the
    ``l4_sum`` tensor passed in (complemented L4 sums) or None."""
    n, nf, dev = _chain(arena, frag_off, frag_len, first)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    _call("rns_rx_verify_chain_dev", dev, arena.data_ptr(), arena.numel(), frag_off.data_ptr(), frag_len.data_ptr(),
          nf, first.data_ptr(), n, ip4, ip6, status.data_ptr(), _per_packet(l4_sum, "l4_sum", n, dev))
    return status, l4_sum


def rx_verify_packed(arena: torch.Tensor, blk_off: torch.Tensor, len16: torch.Tensor, local_ipv4: bytes,
                     local_ipv6: bytes, *, align_log2: int = 4, status: torch.Tensor | None = None,
                     l4_sum: torch.Tensor | None = None) -> torch.Tensor:
    """Receive verify of a PACKED arena of datagrams (rns_rx_verify_packed_dev: u16 lengths,
    one offset per 64 datagrams, 16-byte-aligned starts): the same uint8 status per datagram
    as rx_verify."""
    n, dev = _packed(arena, blk_off, len16, align_log2, None)  # align_log2 (4..12): the C ABI's check
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    _call("rns_rx_verify_packed_dev", dev, arena.data_ptr(), arena.numel(), blk_off.data_ptr(), len16.data_ptr(),
          int(align_log2), n, ip4, ip6, status.data_ptr(), _per_packet(l4_sum, "l4_sum", n, dev))
    return status


def rx_verify_strided(arena: torch.Tensor, stride: int, len16: torch.Tensor, local_ipv4: bytes, local_ipv6: bytes,
                      *, first_off: int = 0, status: torch.Tensor | None = None,
                      l4_sum: torch.Tensor | None = None) -> torch.Tensor:
    """Receive verify of datagrams at a fixed stride (rns_rx_verify_strided_dev): datagram i
    = ``arena[first_off + i*stride : + len16[i]]``, a ring of fixed-size receive slots.  The
    same uint8 status per datagram as rx_verify."""
    dev = _descriptors(arena, ("len16", len16, _U16))
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    if not (0 <= int(first_off) < 2 ** 64 and 0 <= int(stride) < 2 ** 64):
        raise ValueError("first_off and stride must be u64")
    n = len16.numel()
    if n >= 2 ** 32:
        raise ValueError("at most 2^32-1 datagrams per call")
    status = _status(status, n, dev)
    _call("rns_rx_verify_strided_dev", dev, arena.data_ptr(), arena.numel(), int(first_off), int(stride),
          len16.data_ptr(), n, ip4, ip6, status.data_ptr(), _per_packet(l4_sum, "l4_sum", n, dev))
    return status


def tx_fill_packed(arena: torch.Tensor, blk_off: torch.Tensor, len16: torch.Tensor, *, align_log2: int = 4,
                   status: torch.Tensor | None = None, len_hint: int = 0) -> torch.Tensor:
    """Transmit finalize of a PACKED arena of outgoing datagrams (rns_tx_fill_packed_dev: u16
    lengths, one offset per 64 datagrams, starts at 2^align_log2 boundaries, align_log2 >= 4):
    the bytes and the uint8 status per datagram of ``tx_fill``."""
    n, dev = _packed(arena, blk_off, len16, align_log2, (4, 12))
    status = _status(status, n, dev)
    _call("rns_tx_fill_packed_dev", dev, arena.data_ptr(), arena.numel(), blk_off.data_ptr(), len16.data_ptr(),
          int(align_log2), n, status.data_ptr(), int(len_hint))
    return status


def tx_fill_chain(arena: torch.Tensor, frag_off: torch.Tensor, frag_len: torch.Tensor, first: torch.Tensor, *,
                  status: torch.Tensor | None = None) -> torch.Tensor:
    """Transmit finalize of datagrams held as NetBuffer chains (rns_tx_fill_chain_dev):
    datagram i = fragments ``first[i] .. first[i+1]`` as for ``csum_chain``, its FIRST
    fragment the head alloc_header built (the IP header, then the L4 header: buf.rs:262-291),
    the rest its payload.  The L4 checksum over [head[hdr:], payload...] (folded per fragment,
    tcp.rs:957-973, udp.rs:151-171, icmp.rs:87-112) and the IPv4 header checksum
    (ip.rs:140-160) are stored into the head.  Returns a uint8 status per datagram (RNS_TX_*)."""
    n, nf, dev = _chain(arena, frag_off, frag_len, first)
    status = _status(status, n, dev)
    _call("rns_tx_fill_chain_dev", dev, arena.data_ptr(), arena.numel(), frag_off.data_ptr(), frag_len.data_ptr(), nf,
          first.data_ptr(), n, status.data_ptr())
    return status


def tx_chain_packed_layout(head_len, pay_len, pay_align_log2: int = 4, head_first_off: int = 0,
                           pay_first_off: int = 0):
    """Offsets of the compact chain form (rns_tx_chain_packed_layout): heads back to back from
    ``head_first_off``, payloads at 2**pay_align_log2 steps from ``pay_first_off`` (a zero-length
    payload occupies nothing).  ``head_len`` <= 255, ``pay_len`` <= 65535.  Returns
    (head_blk_off uint64 [ceil(n/64)], pay_blk_off uint64 [ceil(n/64)], head_off uint64 [n],
    pay_off uint64 [n], head_end, pay_end)."""
    hl, pl = np.asarray(head_len), np.asarray(pay_len)
    if hl.shape != pl.shape or hl.ndim != 1:
        raise ValueError("head_len and pay_len must be 1-D and of the same size")
    if hl.size and (int(hl.max()) > 0xFF or int(hl.min()) < 0):
        raise ValueError("the compact chain form holds u8 head lengths (<= 255)")
    if pl.size and (int(pl.max()) > 0xFFFF or int(pl.min()) < 0):
        raise ValueError("the compact chain form holds u16 payload lengths (<= 65535)")
    if not 4 <= int(pay_align_log2) <= 12:
        raise ValueError("the compact chain form needs pay_align_log2 in 4..12")
    h8 = np.ascontiguousarray(hl, dtype=np.uint8)
    p16 = np.ascontiguousarray(pl, dtype=np.uint16)
    n = int(h8.size)
    nb = (n + 63) // 64
    hblk, pblk = np.zeros(max(nb, 1), dtype=np.uint64), np.zeros(max(nb, 1), dtype=np.uint64)
    hoff, poff = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    hend, pend = ctypes.c_uint64(0), ctypes.c_uint64(0)
    st = _lib.load().rns_tx_chain_packed_layout(h8.ctypes.data, p16.ctypes.data, n, int(pay_align_log2),
                                                int(head_first_off), int(pay_first_off), hblk.ctypes.data,
                                                pblk.ctypes.data, hoff.ctypes.data, poff.ctypes.data,
                                                ctypes.byref(hend), ctypes.byref(pend))
    _lib.check(st, "rns_tx_chain_packed_layout")
    return hblk[:nb], pblk[:nb], hoff[:n], poff[:n], int(hend.value), int(pend.value)


def tx_fill_chain_packed(arena: torch.Tensor, head_blk_off: torch.Tensor, head_len8: torch.Tensor,
                         pay_blk_off: torch.Tensor, pay_len16: torch.Tensor, *, pay_align_log2: int = 4,
                         status: torch.Tensor | None = None) -> torch.Tensor:
    """Transmit finalize of [head, payload] chains over COMPACT descriptors
    (rns_tx_fill_chain_packed_dev): u8 head lengths and u16 payload lengths (0 = head only), one
    head offset and one payload offset per 64 datagrams (see ``tx_chain_packed_layout``) — 3 B per
    datagram + 16 B per 64 instead of the CSR form's 28 B.  The bytes and the uint8 status per
    datagram of ``tx_fill_chain`` on the chains the lengths imply."""
    dev = _descriptors(arena, ("head_blk_off", head_blk_off, _I64), ("head_len8", head_len8, _U8),
                       ("pay_blk_off", pay_blk_off, _I64), ("pay_len16", pay_len16, _U16))
    n = head_len8.numel()
    if pay_len16.numel() != n:
        raise ValueError("head_len8 and pay_len16 must have one entry per datagram each")
    if head_blk_off.numel() < (n + 63) // 64 or pay_blk_off.numel() < (n + 63) // 64:
        raise ValueError("head_blk_off and pay_blk_off need one offset per 64 datagrams")
    if not 4 <= pay_align_log2 <= 12:
        raise ValueError("the compact chain finalize needs pay_align_log2 in 4..12")
    if n > _lib.RNS_CHAIN_MAX_PACKETS:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} datagrams per chain call")
    status = _status(status, n, dev)
    _call("rns_tx_fill_chain_packed_dev", dev, arena.data_ptr(), arena.numel(), head_blk_off.data_ptr(),
          head_len8.data_ptr(), pay_blk_off.data_ptr(), pay_len16.data_ptr(), int(pay_align_log2), n,
          status.data_ptr())
    return status


def tx_fill(arena: torch.Tensor, off: torch.Tensor, length: torch.Tensor, *,
            status: torch.Tensor | None = None) -> torch.Tensor:
    """Transmit finalize of a batch of outgoing IP datagrams (rns_tx_fill_dev): the
    IPv4 header checksum and the TCP / UDP / ICMP checksum of every datagram stored in
    place, pseudo-headers formed on the device (tcp.rs:957-973, udp.rs:151-171,
    icmp.rs:87-112, ip.rs:140-160).  Returns a uint8 status per datagram (RNS_TX_*)."""
    n, dev = _explicit(arena, off, length)
    status = _status(status, n, dev)
    _call("rns_tx_fill_dev", dev, arena.data_ptr(), arena.numel(), off.data_ptr(), length.data_ptr(), n,
          status.data_ptr())
    return status


def fill_splitmix64(buf: torch.Tensor, seed: int) -> torch.Tensor:
    """Fill a device uint8 buffer with the splitmix64 byte stream (same bytes as
    oracle.splitmix64_bytes(seed, n))."""
    _require_cuda(buf, "buf", _U8)
    _call("rns_fill_splitmix64_dev", buf.device, buf.data_ptr(), buf.numel(), seed & 0xFFFFFFFFFFFFFFFF)
    return buf


def recv_batch(fd: int, arena: np.ndarray, slot_bytes: int = 2048, max_pkts: int | None = None,
               timeout_ms: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Read every queued datagram (after waiting up to ``timeout_ms`` for the first)
    into consecutive ``slot_bytes`` slots of ``arena`` (rns_io_recv_batch; the batched
    form of recv_packet, netif.rs:65-83).  Returns (offsets uint64, lengths uint32)."""
    if arena.dtype != np.uint8 or not arena.flags["C_CONTIGUOUS"]:
        raise ValueError("arena must be a contiguous uint8 array")
    cap = arena.shape[0] // slot_bytes
    max_pkts = cap if max_pkts is None else min(max_pkts, cap)
    off = np.empty(max(max_pkts, 1), dtype=np.uint64)
    ln = np.empty(max(max_pkts, 1), dtype=np.uint32)
    r = _lib.load().rns_io_recv_batch(int(fd), arena.ctypes.data, slot_bytes, max_pkts, off.ctypes.data,
                                      ln.ctypes.data, int(timeout_ms))
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_recv_batch")
    return off[:r], ln[:r]


def recv_batch_packed(fd: int, arena: np.ndarray, mru: int = 2048, max_pkts: int | None = None,
                      timeout_ms: int = 0) -> tuple[np.ndarray, np.ndarray, int]:
    """Read every queued datagram (after waiting up to ``timeout_ms`` for the first) into
    ``arena`` PACKED: each at the next 16-byte boundary while a datagram of ``mru`` bytes
    still fits (rns_io_recv_batch_packed).  Returns (lengths uint16 [n], blk_off uint64
    [ceil(n/64)], end) — the packed form's descriptors (rx_verify_packed) and the bytes used."""
    if arena.dtype != np.uint8 or not arena.flags["C_CONTIGUOUS"]:
        raise ValueError("arena must be a contiguous uint8 array")
    if not 0 < int(mru) <= 0xFFFF:
        raise ValueError("mru must be in 1..65535 (the packed form's lengths are u16)")
    cap = arena.shape[0] // 16  # no more datagrams than 16-byte slots
    max_pkts = cap if max_pkts is None else min(int(max_pkts), cap)
    max_pkts = min(max_pkts, 2 ** 31 - 1)
    ln = np.empty(max(max_pkts, 1), dtype=np.uint16)
    blk = np.empty(max((max_pkts + 63) // 64, 1), dtype=np.uint64)
    end = ctypes.c_uint64(0)
    if max_pkts <= 0:
        return ln[:0], blk[:0], 0
    r = _lib.load().rns_io_recv_batch_packed(int(fd), arena.ctypes.data, arena.shape[0], int(mru), max_pkts,
                                             ln.ctypes.data, blk.ctypes.data, ctypes.byref(end), int(timeout_ms))
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_recv_batch_packed")
    return ln[:r], blk[:(r + 63) // 64], int(end.value)


def _recv_chain_args(pool: np.ndarray, free: np.ndarray, buf_bytes: int, mru: int, max_pkts: int | None):
    """The checks recv_batch_chain and recv_batch_pool share: (buf_bytes, mru, n_free, max_pkts)."""
    if pool.dtype != np.uint8 or not pool.flags["C_CONTIGUOUS"]:
        raise ValueError("pool must be a contiguous uint8 array")
    if free.dtype != np.uint32 or not free.flags["C_CONTIGUOUS"] or not free.flags["WRITEABLE"]:
        raise ValueError("free must be a contiguous writable uint32 array (it is permuted in place)")
    buf_bytes, mru = int(buf_bytes), int(mru)
    if buf_bytes <= 0 or mru <= 0 or mru >= 2 ** 32:
        raise ValueError("buf_bytes and mru must be positive")
    need = -(-mru // buf_bytes)
    if need > _lib.RNS_IO_MAX_FRAGS:
        raise ValueError(f"a datagram of mru bytes may take at most {_lib.RNS_IO_MAX_FRAGS} buffers")
    n_free = free.shape[0]
    if n_free and int(free.max()) >= pool.shape[0] // buf_bytes:
        raise ValueError("free names a buffer outside the pool")
    cap = max(n_free - need + 1, 0)  # a datagram keeps at least one buffer and is offered `need`
    max_pkts = cap if max_pkts is None else min(int(max_pkts), cap)
    return buf_bytes, mru, n_free, min(max_pkts, 2 ** 31 - 1)


def recv_batch_chain(fd: int, pool: np.ndarray, free: np.ndarray, buf_bytes: int = 512, mru: int = 2048,
                     max_pkts: int | None = None, timeout_ms: int = 0):
    """Read every queued datagram (after waiting up to ``timeout_ms`` for the first) into
    NetBuffer chains (rns_io_recv_batch_chain; batched recv_packet, netif.rs:65-83): ``pool`` is
    a uint8 pool of ``buf_bytes``-byte buffers, ``free`` (uint32, contiguous, permuted IN PLACE)
    the indices of the free ones.  Each datagram is offered ``ceil(mru / buf_bytes)`` buffers and
    keeps those it filled.  Returns ``(n, frag_off uint64, frag_len uint32, first uint32 [n+1],
    n_frags)``: on return ``free[:n_frags]`` are the buffers in use, in fragment order, and
    ``free[n_frags:]`` are still free."""
    buf_bytes, mru, n_free, max_pkts = _recv_chain_args(pool, free, buf_bytes, mru, max_pkts)
    frag_off = np.empty(max(n_free, 1), dtype=np.uint64)
    frag_len = np.empty(max(n_free, 1), dtype=np.uint32)
    first = np.zeros(max(max_pkts, 0) + 1, dtype=np.uint32)
    if max_pkts <= 0:
        return 0, frag_off[:0], frag_len[:0], first[:1], 0
    nf = ctypes.c_uint32(0)
    r = _lib.load().rns_io_recv_batch_chain(int(fd), pool.ctypes.data, buf_bytes, free.ctypes.data, n_free, mru,
                                            max_pkts, frag_off.ctypes.data, frag_len.ctypes.data, first.ctypes.data,
                                            ctypes.byref(nf), int(timeout_ms))
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_recv_batch_chain")
    return r, frag_off[:nf.value], frag_len[:nf.value], first[:r + 1], int(nf.value)


def send_batch(fd: int, arena: np.ndarray, off: np.ndarray, length: np.ndarray) -> int:
    """Write one datagram per packet (rns_io_send_batch; batched send_packet, netif.rs:85-98)."""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    length = np.ascontiguousarray(length, dtype=np.uint32)
    r = _lib.load().rns_io_send_batch(int(fd), arena.ctypes.data, off.ctypes.data, length.ctypes.data,
                                      off.shape[0])
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_send_batch")
    return r


def send_batch_chain(fd: int, arena: np.ndarray, frag_off: np.ndarray, frag_len: np.ndarray,
                     first: np.ndarray) -> int:
    """Send NetBuffer chains (rns_io_send_batch_chain; batched send_packet, netif.rs:85-98):
    datagram i = fragments ``first[i] .. first[i+1]`` of ``arena`` gathered into one datagram,
    as to_iovec + tun_send's writev do.  Returns the number of datagrams sent."""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    frag_off = np.ascontiguousarray(frag_off, dtype=np.uint64)
    frag_len = np.ascontiguousarray(frag_len, dtype=np.uint32)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    n = first.shape[0] - 1
    if n < 0 or frag_off.shape[0] != frag_len.shape[0]:
        raise ValueError("first needs n+1 entries; frag_off and frag_len one per fragment")
    if n and int(first[-1]) > frag_off.shape[0]:
        raise ValueError("first points past the fragment arrays")
    if frag_off.shape[0] and int((frag_off + frag_len.astype(np.uint64)).max()) > arena.shape[0]:
        raise ValueError("a fragment lies outside the arena")
    r = _lib.load().rns_io_send_batch_chain(int(fd), arena.ctypes.data, frag_off.ctypes.data, frag_len.ctypes.data,
                                            first.ctypes.data, n)
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_send_batch_chain")
    return r


class PinnedBuffer:
    """Page-locked host memory (rns_host_alloc) viewed as a numpy uint8 array."""

    def __init__(self, nbytes: int):
        lib = _lib.load()
        p = ctypes.c_void_p()
        _lib.check(lib.rns_host_alloc(max(nbytes, 1), ctypes.byref(p)), "rns_host_alloc")
        self.ptr = p.value
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * max(nbytes, 1)).from_address(self.ptr))[:nbytes]

    def free(self) -> None:
        if self.ptr:
            self.array = None
            _lib.load().rns_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBatcher:
    """Host-resident batches: chunked H2D, kernel, D2H of results overlapped on
    ``nstreams`` streams (rns_csum_batch_host).  Offsets must be ascending."""

    _run, _destroy = "rns_csum_batch_host", "rns_host_ctx_destroy"

    def __init__(self, device: int = 0, chunk_bytes: int = 64 << 20, nstreams: int = 3):
        lib = _lib.load()
        ctx = ctypes.c_void_p()
        _lib.check(lib.rns_host_ctx_create(device, chunk_bytes, nstreams, ctypes.byref(ctx)), "rns_host_ctx_create")
        self.ctx = ctx.value

    def run(self, arena: np.ndarray, off: np.ndarray, length: np.ndarray, seed: np.ndarray | None = None,
            complement: bool = False, out: np.ndarray | None = None) -> np.ndarray:
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        n = off.shape[0]
        if out is None:
            out = np.empty(n, dtype=np.uint16)
        sp = None
        if seed is not None:
            seed = np.ascontiguousarray(seed, dtype=np.uint16)
            sp = seed.ctypes.data
        st = getattr(_lib.load(), self._run)(self.ctx, arena.ctypes.data, arena.shape[0], off.ctypes.data,
                                             length.ctypes.data, sp, out.ctypes.data, n, _flags(complement))
        _lib.check(st, self._run)
        return out

    def close(self) -> None:
        if self.ctx:
            getattr(_lib.load(), self._destroy)(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiHostBatcher(HostBatcher):
    """Host-resident batches over several GPUs (rns_csum_batch_multi_host): the
    batch is cut into contiguous packet ranges of about equal bytes, one per entry
    of ``devices`` (a device may repeat), each through its own staging context."""

    _run, _destroy = "rns_csum_batch_multi_host", "rns_multi_ctx_destroy"

    def __init__(self, devices, chunk_bytes: int = 64 << 20, nstreams: int = 3):
        lib = _lib.load()
        devs = (ctypes.c_int * len(devices))(*devices)
        ctx = ctypes.c_void_p()
        _lib.check(lib.rns_multi_ctx_create(devs, len(devices), chunk_bytes, nstreams, ctypes.byref(ctx)),
                   "rns_multi_ctx_create")
        self.ctx = ctx.value
        self.devices = list(devices)


def csum_batch_multi_dev(shards, *, complement: bool = False) -> None:
    """Launch every GPU's shard (rns_csum_batch_multi_dev).  ``shards``: a sequence of
    dicts with keys arena, off, length, out (torch tensors on that shard's device)
    and optional seed, len_hint, stream.  Asynchronous on each device's stream."""
    arr = (_lib.RnsDevBatch * len(shards))()
    keep = []
    for k, sh in enumerate(shards):
        arena, off, length, out = sh["arena"], sh["off"], sh["length"], sh["out"]
        seed = sh.get("seed")
        for t, name, dt in ((arena, "arena", (torch.uint8,)), (off, "off", (torch.int64,)),
                            (length, "length", (torch.int32,)), (out, "out", _U16)):
            _require_cuda(t, name, dt)
        if seed is not None:
            _require_cuda(seed, "seed", _U16)
        n = off.shape[0]
        if length.shape[0] != n or out.shape[0] < n or (seed is not None and seed.shape[0] < n):
            raise ValueError(f"shard {k}: descriptor arrays disagree in length")
        dev = arena.device.index
        if any(t.device != arena.device for t in (off, length, out)):
            raise ValueError(f"shard {k}: tensors on different devices")
        stream = sh.get("stream")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        hint = sh.get("len_hint")
        if hint is None:
            hint = int(length.float().mean().item()) if n else 0
        arr[k] = _lib.RnsDevBatch(dev, arena.data_ptr(), arena.numel(), off.data_ptr(), length.data_ptr(),
                                  seed.data_ptr() if seed is not None else None, out.data_ptr(), n, hint, None,
                                  stream.cuda_stream)
        keep.append(sh)
    flags = _lib.RNS_FLAG_COMPLEMENT if complement else 0
    _lib.check(_lib.load().rns_csum_batch_multi_dev(arr, len(shards), flags), "rns_csum_batch_multi_dev")


# The pool-buffer receive and transmit paths (pool.py builds on the checks above) are part of this
# module's interface: batch.rx_pool_layout, batch.rx_verify_pool, batch.recv_batch_pool,
# batch.tx_pool_layout, batch.tx_fill_pool, batch.send_batch_pool.
_POOL_API = ("recv_batch_pool", "rx_pool_layout", "rx_verify_pool", "send_batch_pool", "tx_fill_pool", "tx_pool_layout")
# and so is TCP segmentation offload (segment.py): batch.tx_segment, batch.tx_segment_layout, batch.tx_segment_chains.
_SEGMENT_API = ("tx_segment", "tx_segment_chains", "tx_segment_layout")
# and TCP receive placement (place.py): batch.rx_tcp_place_pool, batch.rx_flow_table, batch.Reassembler, batch.META_DTYPE.
_PLACE_API = ("META_DTYPE", "Reassembler", "meta_records", "rx_flow_table", "rx_tcp_place_pool")
# and the TCP flow update and ACK build (flow.py): batch.rx_tcp_flow_update, batch.tx_ack_build, batch.flow_update_host.
_FLOW_API = ("FLOW_DTYPE", "RES_DTYPE", "SEG_DTYPE", "flow_update_host", "flow_update_work", "rx_tcp_flow_update",
             "tx_ack_build")
# and TCP send planning (send.py): batch.tx_tcp_plan, batch.tx_tcp_send, batch.plan_host, batch.tx_plan_work,
# batch.PLAN_RES_DTYPE (send.RES_DTYPE: RES_DTYPE here is the flow update's).
_SEND_API = ("PLAN_RES_DTYPE", "plan_host", "tx_plan_work", "tx_tcp_plan", "tx_tcp_send")
# and the ICMP echo responder (icmp.py): batch.rx_icmp_echo_pool, batch.echo_host, batch.echo_respond, batch.echo_work.
_ICMP_API = ("echo_host", "echo_respond", "echo_work", "rx_icmp_echo_pool")
# and the UDP receive demux (udp.py): batch.rx_udp_demux_pool, batch.demux_host, batch.drain, batch.udp_demux,
# batch.port_table, batch.demux_work — and its send build: batch.tx_udp_send_pool, batch.send_host,
# batch.udp_send_work, batch.udp_echo, batch.UdpSend.
_UDP_API = ("demux_host", "demux_work", "drain", "port_table", "rx_udp_demux_pool", "udp_demux",
            "UdpSend", "send_host", "tx_udp_send_pool", "udp_echo", "udp_send_work")
# and the TCP listen responder (listen.py): batch.rx_tcp_listen_pool, batch.listen_host, batch.listen_work,
# batch.tcp_listen, batch.accept_merge, batch.TcpListen.
_LISTEN_API = ("TcpListen", "accept_merge", "listen_host", "listen_work", "rx_tcp_listen_pool", "tcp_listen")
# and the TCP connection update, control-segment build and close step (conn.py): batch.rx_tcp_conn_update,
# batch.tx_tcp_ctl_build, batch.tx_tcp_close, batch.conn_work, batch.conn_update_host, batch.ctl_heads_host,
# batch.close_host, batch.tcp_conn, batch.CTL_DTYPE.
_CONN_API = ("CTL_DTYPE", "close_host", "conn_update_host", "conn_work", "ctl_heads_host", "rx_tcp_conn_update", "tcp_conn",
             "tx_tcp_close", "tx_tcp_ctl_build")


def __getattr__(name):
    if name in _POOL_API:
        from . import pool
        return getattr(pool, name)
    if name in _SEGMENT_API:
        from . import segment
        return getattr(segment, name)
    if name in _PLACE_API:
        from . import place
        return getattr(place, name)
    if name in _FLOW_API:
        from . import flow
        return getattr(flow, name)
    if name in _SEND_API:
        from . import send
        return getattr(send, name)
    if name in _ICMP_API:
        from . import icmp
        return getattr(icmp, name)
    if name in _UDP_API:
        from . import udp
        return getattr(udp, name)
    if name in _LISTEN_API:
        from . import listen
        return getattr(listen, name)
    if name in _CONN_API:
        from . import conn
        return getattr(conn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
