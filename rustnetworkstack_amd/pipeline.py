"""End-to-end batched receive and transmit.

Receive (RxPipeline): datagram fd -> pinned host arena -> HBM -> fused receive verify
-> per-packet verdicts.  By default the datagrams are received PACKED (each at the next
16-byte boundary, rns_io_recv_batch_packed), so the copy to the GPU carries their bytes
only — not whole 2048-byte slots — and the verify is the rows receive kernel
(rns_rx_verify_packed_dev); ``packed=False`` keeps MRU slots and rns_rx_verify_dev.  Transmit (TxPipeline): pinned slots -> HBM -> transmit
finalize -> the changed header bytes back -> datagram fd.  TxChainPipeline does the same for
datagrams built as the reference builds them — NetBuffer chains of a head fragment (IP + L4
headers) and a payload — with the heads in a header region and the payloads in a payload region:
only used bytes cross PCIe to the GPU, only the header region comes back, and each datagram leaves
gathered from its two fragments (rns_io_send_batch_chain, like send_packet's writev).
RxPoolPipeline receives as the reference does — into a pool of fixed-size buffers that stay held
until the stack releases them (rns_io_recv_batch_pool) — and verifies the chains where they lie
(rns_rx_verify_pool_dev): a batch costs one copy of the buffers it used and 14 B of descriptors per
MTU datagram.  TxPoolPipeline is its transmit twin: datagrams built in the pool as tcp_output
builds them (a head buffer with the headers at its end, payload buffers filled from their start)
are finalized where they lie (rns_tx_fill_pool_dev), only the heads' tails come back, and each
leaves gathered from its buffers (rns_io_send_batch_pool).  TxSegmentPipeline moves tcp_write's
segment loop to the device: per send one template head, the data where it lies and the mss go up,
rns_tx_segment_dev builds and finalizes every segment's head, and only the header region comes back.

The reference handles one packet per loop iteration on its receive thread
(packet_receive_thread lib.rs:26-31 -> recv_packet netif.rs:65-83 -> ip_input
ip.rs:38 -> checks ip.rs:76, tcp.rs:544).  Here one call moves every queued datagram
(rns_io_recv_batch into 2048-byte MRU slots, netif.rs:66), copies the used slots to
the GPU in one transfer and verifies them with one kernel (rns_rx_verify_dev).

Both directions also run overlapped (``RxPipeline.stream``, ``TxPipeline.submit`` /
``complete``): two buffer sets, the GPU work of one batch (H2D, kernel, D2H into
pinned memory) queued on a private stream while the host reads or writes the
datagrams of the other.
"""
from __future__ import annotations

from collections import deque
from typing import Iterator

import numpy as np
import torch

from .batch import (PinnedBuffer, recv_batch, recv_batch_packed, rx_verify, rx_verify_packed, send_batch,
                    send_batch_chain, tx_fill, tx_fill_chain, tx_fill_chain_packed)
from .pool import _buf_log2, recv_batch_pool, rx_verify_pool, send_batch_pool, tx_fill_pool, tx_pool_layout
from .segment import tx_segment, tx_segment_chains, tx_segment_layout

MRU = 2048  # netif.rs:66


class _Slots:
    """One buffer set: pinned host slots + lengths + per-slot results, and their HBM twins
    (packed: u16 lengths and one block offset per 64 datagrams instead of u32 lengths)."""

    def __init__(self, dev: torch.device, max_pkts: int, slot_bytes: int, head: int = 0, packed: bool = False):
        self.host = PinnedBuffer(slot_bytes * max_pkts)
        self.h_len = PinnedBuffer(4 * max_pkts)
        self.h_status = PinnedBuffer(max_pkts)
        self.h_head = PinnedBuffer(head * max_pkts) if head else None
        self.d_arena = torch.empty(slot_bytes * max_pkts, dtype=torch.uint8, device=dev)
        self.d_len = torch.empty(max_pkts, dtype=torch.int32, device=dev)
        self.d_status = torch.empty(max_pkts, dtype=torch.uint8, device=dev)
        nblk = (max_pkts + 63) // 64
        self.h_blk = PinnedBuffer(8 * nblk) if packed else None
        self.d_blk = torch.empty(nblk, dtype=torch.int64, device=dev) if packed else None
        self.done = torch.cuda.Event()

    def close(self):
        for b in (self.host, self.h_len, self.h_status, self.h_head, self.h_blk):
            if b is not None:
                b.free()


class Datagrams:
    """The datagrams of one received batch: ``d[i]`` is datagram i's bytes (a view of the
    pinned arena, valid until the buffer set is reused)."""

    def __init__(self, arena: np.ndarray, off: np.ndarray, length: np.ndarray):
        self.arena, self.off, self.length = arena, off, length

    def __len__(self) -> int:
        return int(self.length.shape[0])

    def __getitem__(self, i: int) -> np.ndarray:
        o = int(self.off[i])
        return self.arena[o:o + int(self.length[i])]


class RxPipeline:
    def __init__(self, local_ipv4: bytes, local_ipv6: bytes, device: int = 0, max_pkts: int = 65536,
                 slot_bytes: int = MRU, packed: bool = True):
        self.local_ipv4, self.local_ipv6 = bytes(local_ipv4), bytes(local_ipv6)
        self.slot = slot_bytes  # the MRU: the arena holds max_pkts datagrams of this size
        self.max_pkts = max_pkts
        self.packed = packed
        self.dev = torch.device(f"cuda:{device}")
        self._sets = [_Slots(self.dev, max_pkts, slot_bytes, packed=packed)]
        self.d_off = (torch.arange(max_pkts, dtype=torch.int64, device=self.dev) * slot_bytes).contiguous()
        self._stream = None
        self.h2d_bytes = 0  # arena bytes copied to the GPU so far (packed: the datagrams' 16-byte-padded bytes)
        self.datagrams = 0
        self.last: Datagrams | None = None  # the datagrams of the last batch ``receive`` returned

    @property
    def host(self) -> PinnedBuffer:
        """Set 0's pinned arena: where ``receive`` leaves its datagrams (``last``)."""
        return self._sets[0].host

    def _read(self, s: _Slots, fd: int, timeout_ms: int):
        """One batched read into set ``s``: (lengths, Datagrams, arena bytes used)."""
        if self.packed:
            ln16, blk, end = recv_batch_packed(fd, s.host.array, self.slot, self.max_pkts, timeout_ms)
            n = ln16.shape[0]
            if n:
                s.h_blk.array.view(np.uint64)[: blk.shape[0]] = blk
            pad = (ln16.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)
            off = np.zeros(n, dtype=np.uint64)
            if n > 1:
                np.cumsum(pad[:-1], out=off[1:])
            return ln16.astype(np.uint32), Datagrams(s.host.array, off, ln16), end
        off, ln = recv_batch(fd, s.host.array, self.slot, self.max_pkts, timeout_ms)
        return ln, Datagrams(s.host.array, off, ln), ln.shape[0] * self.slot

    def _submit(self, s: _Slots, ln: np.ndarray, used: int) -> None:
        """Queue H2D + verify + status D2H of the batch in ``s`` (len(ln) datagrams in its
        first ``used`` arena bytes) on the current stream; ``s.done`` marks the status
        landing in pinned memory."""
        n = ln.shape[0]
        # pinned host memory (rns_host_alloc): every copy is a DMA transfer
        s.d_arena[:used].copy_(torch.from_numpy(s.host.array[:used]), non_blocking=True)
        self.h2d_bytes += used
        self.datagrams += n
        if self.packed:
            h16 = s.h_len.array.view(np.uint16)[:n]
            h16[:] = ln
            nb = (n + 63) // 64
            d16 = s.d_len.view(torch.int16)[:n]
            d16.copy_(torch.from_numpy(h16.view(np.int16)), non_blocking=True)
            s.d_blk[:nb].copy_(torch.from_numpy(s.h_blk.array.view(np.int64)[:nb]), non_blocking=True)
            rx_verify_packed(s.d_arena[:max(used, 1)], s.d_blk[:nb], d16, self.local_ipv4, self.local_ipv6,
                             status=s.d_status[:n])
        else:
            hl = s.h_len.array.view(np.uint32)[:n]
            hl[:] = ln
            s.d_len[:n].copy_(torch.from_numpy(hl.view(np.int32)), non_blocking=True)
            rx_verify(s.d_arena, self.d_off[:n], s.d_len[:n], self.local_ipv4, self.local_ipv6,
                      status=s.d_status[:n])
        torch.from_numpy(s.h_status.array[:n]).copy_(s.d_status[:n], non_blocking=True)
        s.done.record()

    def receive(self, fd: int, timeout_ms: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """One batch: returns (status uint8 [n], lengths uint32 [n]); ``self.last[i]`` is
        datagram i's bytes in the pinned arena."""
        s = self._sets[0]
        ln, dg, used = self._read(s, fd, timeout_ms)
        self.last = dg
        n = ln.shape[0]
        if n == 0:
            return np.empty(0, dtype=np.uint8), ln
        with torch.cuda.device(self.dev):
            self._submit(s, ln, used)
            s.done.synchronize()
        return s.h_status.array[:n].copy(), ln

    def stream(self, fd: int, timeout_ms: int = 0) -> Iterator[tuple[np.ndarray, np.ndarray, Datagrams]]:
        """Overlapped receive: yields (status [n], lengths [n], Datagrams) per batch until a
        read finds nothing within ``timeout_ms``.  While batch k is on the GPU the host reads
        batch k+1 into the other buffer set; the yielded arrays stay valid until the
        generator is resumed."""
        if len(self._sets) == 1:
            self._sets.append(_Slots(self.dev, self.max_pkts, self.slot, packed=self.packed))
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.dev)
        pending = None  # (set, lengths, datagrams) on the GPU
        k = 0
        while True:
            s = self._sets[k]
            if pending is None:
                ln, dg, used = self._read(s, fd, timeout_ms)
            else:
                # take what is queued now (no wait), hand the finished batch over, and
                # only then block for more: the last batch is not held back by the timeout
                ln, dg, used = self._read(s, fd, 0)
                p, pln, pdg = pending
                p.done.synchronize()
                yield p.h_status.array[: pln.shape[0]], pln, pdg
                pending = None
                if ln.shape[0] == 0:
                    ln, dg, used = self._read(s, fd, timeout_ms)
            if ln.shape[0] == 0:
                return
            with torch.cuda.device(self.dev), torch.cuda.stream(self._stream):
                self._submit(s, ln, used)
            pending = (s, ln, dg)
            k ^= 1

    def close(self):
        for s in self._sets:
            s.close()


class TxPipeline:
    """End-to-end batched transmit (transmit side): the caller builds
    datagrams in pinned MRU slots with their checksum fields unset (what tcp_output /
    udp_output / icmp_output_* and ip_output_v4 hand over before their checksum step)
    -> one H2D copy -> rns_tx_fill_dev (IPv4 header + L4 checksums, pseudo-headers on the
    device) -> D2H of each slot's first HEAD bytes (every byte the fill can change)
    -> rns_io_send_batch (one writev per datagram, like tun_send via send_packet,
    netif.rs:85-98).

    ``send`` does one batch synchronously.  ``submit`` / ``complete`` overlap: submit
    queues a batch's GPU work and returns; complete waits for the oldest submitted
    batch and writes it to the fd.  With two buffer sets, the caller fills the next
    batch's ``slots()`` and the host sends one batch while the GPU finalizes the other:

        for lengths in batches:
            if pipe.pending() == pipe.DEPTH:
                statuses.append(pipe.complete(fd))
            fill(pipe.slots(), ...)
            pipe.submit(lengths)
        while pipe.pending():
            statuses.append(pipe.complete(fd))
    """

    HEAD = 128  # the fill writes only below byte 96 of a slot-aligned datagram
    DEPTH = 2

    def __init__(self, device: int = 0, max_pkts: int = 65536, slot_bytes: int = MRU):
        self.slot = slot_bytes
        self.max_pkts = max_pkts
        self.dev = torch.device(f"cuda:{device}")
        self._sets = [_Slots(self.dev, max_pkts, slot_bytes, head=self.HEAD) for _ in range(self.DEPTH)]
        self.d_off = (torch.arange(max_pkts, dtype=torch.int64, device=self.dev) * slot_bytes).contiguous()
        self.off = np.arange(max_pkts, dtype=np.uint64) * np.uint64(slot_bytes)
        self._next = 0                    # the set slots() hands out
        self._inflight: deque = deque()   # (set, lengths), oldest first
        self._stream = None

    def slots(self) -> np.ndarray:
        """The free set's pinned slots, shape (max_pkts, slot_bytes): datagram i goes in row i."""
        if len(self._inflight) == self.DEPTH:
            raise RuntimeError("every buffer set is in flight: complete() one first")
        return self._sets[self._next].host.array[: self.slot * self.max_pkts].reshape(self.max_pkts, self.slot)

    def pending(self) -> int:
        return len(self._inflight)

    def _check(self, lengths: np.ndarray) -> np.ndarray:
        n = int(lengths.shape[0])
        if n > self.max_pkts:
            raise ValueError("more datagrams than slots")
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        if n and int(ln.max()) > self.slot:
            raise ValueError("datagram longer than its slot")
        return ln

    def _queue(self, s: _Slots, ln: np.ndarray) -> None:
        n = ln.shape[0]
        hl = s.h_len.array.view(np.uint32)[:n]
        hl[:] = ln
        head = s.h_head.array[: self.HEAD * n].reshape(n, self.HEAD)
        s.d_arena[: n * self.slot].copy_(torch.from_numpy(s.host.array[: n * self.slot]), non_blocking=True)
        s.d_len[:n].copy_(torch.from_numpy(hl.view(np.int32)), non_blocking=True)
        tx_fill(s.d_arena, self.d_off[:n], s.d_len[:n], status=s.d_status[:n])
        heads = s.d_arena[: n * self.slot].view(n, self.slot)[:, : self.HEAD].contiguous()
        torch.from_numpy(head).copy_(heads, non_blocking=True)
        torch.from_numpy(s.h_status.array[:n]).copy_(s.d_status[:n], non_blocking=True)
        s.done.record()

    def _finish(self, fd: int, s: _Slots, ln: np.ndarray) -> np.ndarray:
        n = ln.shape[0]
        s.done.synchronize()
        slots = s.host.array[: self.slot * n].reshape(n, self.slot)
        slots[:, : self.HEAD] = s.h_head.array[: self.HEAD * n].reshape(n, self.HEAD)
        sent = send_batch(fd, s.host.array, self.off[:n], ln)
        if sent != n:
            raise OSError(f"sent {sent} of {n} datagrams")
        return s.h_status.array[:n].copy()

    def send(self, fd: int, lengths: np.ndarray) -> np.ndarray:
        """Fill and send the datagrams in slots [0, n) of ``slots()``; returns their
        RNS_TX_* status."""
        if self._inflight:
            raise RuntimeError("submitted batches pending: complete() them first")
        ln = self._check(lengths)
        if ln.shape[0] == 0:
            return np.empty(0, dtype=np.uint8)
        s = self._sets[self._next]
        with torch.cuda.device(self.dev):
            self._queue(s, ln)
        return self._finish(fd, s, ln)

    def submit(self, lengths: np.ndarray) -> None:
        """Queue the GPU work for slots [0, n) of ``slots()`` and hand out the other set."""
        if len(self._inflight) == self.DEPTH:
            raise RuntimeError("every buffer set is in flight: complete() one first")
        ln = self._check(lengths)
        s = self._sets[self._next]
        with torch.cuda.device(self.dev):
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.dev)
            with torch.cuda.stream(self._stream):
                if ln.shape[0]:
                    self._queue(s, ln)
                else:
                    s.done.record()
        self._inflight.append((s, ln))
        self._next = (self._next + 1) % self.DEPTH

    def complete(self, fd: int) -> np.ndarray:
        """Wait for the oldest submitted batch, send it; returns its RNS_TX_* status."""
        if not self._inflight:
            raise RuntimeError("nothing submitted")
        s, ln = self._inflight.popleft()
        if ln.shape[0] == 0:
            return np.empty(0, dtype=np.uint8)
        return self._finish(fd, s, ln)

    def close(self):
        for s in self._sets:
            s.close()


class _ChainSet:
    """One buffer set of TxChainPipeline: a pinned arena [header region | payload region], its
    chain descriptors and statuses, and their HBM twins (the same offsets on both sides)."""

    def __init__(self, dev: torch.device, max_pkts: int, head_region: int, payload_bytes: int,
                 compact: bool = False):
        # the compact descriptors of a batch in one buffer: [head_blk_off | pay_blk_off | pay_len16 | head_len8]
        cbytes = compact_desc_bytes(max_pkts)
        self.h_cdesc = PinnedBuffer(cbytes) if compact else None
        self.d_cdesc = torch.empty(cbytes, dtype=torch.uint8, device=dev) if compact else None
        self.host = PinnedBuffer(head_region + payload_bytes)
        self.h_off = PinnedBuffer(8 * 2 * max_pkts)
        self.h_len = PinnedBuffer(4 * 2 * max_pkts)
        self.h_first = PinnedBuffer(4 * (max_pkts + 1))
        self.h_status = PinnedBuffer(max_pkts)
        self.d_arena = torch.empty(head_region + payload_bytes, dtype=torch.uint8, device=dev)
        self.d_off = torch.empty(2 * max_pkts, dtype=torch.int64, device=dev)
        self.d_len = torch.empty(2 * max_pkts, dtype=torch.int32, device=dev)
        self.d_first = torch.empty(max_pkts + 1, dtype=torch.int32, device=dev)
        self.d_status = torch.empty(max_pkts, dtype=torch.uint8, device=dev)
        self.cform = False  # the batch described last takes the compact route
        self.done = torch.cuda.Event()

    def close(self):
        for b in (self.host, self.h_off, self.h_len, self.h_first, self.h_status, self.h_cdesc):
            if b is not None:
                b.free()


def compact_desc_bytes(n: int) -> int:
    """Bytes of a batch's compact chain descriptors: 3 B per datagram + 16 B per 64 datagrams."""
    return 3 * n + 16 * ((n + 63) // 64)


def chain_compact_form(head_len, pay_off, pay_len, pay_base: int = 0):
    """The compact descriptors (rns_tx_fill_chain_packed_dev, 16-byte payload alignment) of a
    batch of [head, payload] datagrams whose heads lie back to back from arena offset 0 and whose
    payloads lie at ``pay_base + pay_off``, or None when the payload offsets are not exactly the
    packed layout: ascending, each at the 16-byte-aligned end of the previous payload, from a
    16-byte-aligned first offset (the offset of a zero-length payload means nothing and is not
    looked at).  Returns (head_blk_off, head_len8, pay_blk_off, pay_len16) as numpy arrays."""
    hl = np.ascontiguousarray(head_len, dtype=np.int64)
    po = np.ascontiguousarray(pay_off, dtype=np.int64)
    pl = np.ascontiguousarray(pay_len, dtype=np.int64)
    n = hl.shape[0]
    if n == 0 or hl.min() < 0 or hl.max() > 0xFF or pl.min() < 0 or pl.max() > 0xFFFF:
        return None
    pad = (pl + 15) & ~15
    rel = np.cumsum(pad) - pad  # every payload's offset from the first one
    has = pl > 0
    first = 0
    if has.any():
        first = int(po[has][0])
        if first < 0 or (first + pay_base) & 15 or not np.array_equal(po[has], first + rel[has]):
            return None
    # the block offsets rns_tx_chain_packed_layout gives for these lengths (heads from 0, payloads from
    # pay_base + first), taken from the sums already at hand
    hblk = (np.cumsum(hl) - hl)[::64].astype(np.uint64)
    pblk = (rel[::64] + (pay_base + first)).astype(np.uint64)
    return hblk, hl.astype(np.uint8), pblk, pl.astype(np.uint16)


class TxChainPipeline:
    """Batched transmit of NetBuffer chains: the caller writes each
    datagram's head fragment — IP header then L4 header, checksum fields unset, as
    alloc_header leaves them (buf.rs:262-291) — back to back into ``heads()`` and its payload
    at a 16-byte-aligned offset of its choice into ``payloads()``, then ``send`` (or
    ``submit`` / ``complete``) with the head lengths and the payload offsets and lengths.
    One H2D copy of the used header bytes and one of the used payload bytes ->
    rns_tx_fill_chain_dev (pseudo-headers, L4 and IPv4 header checksums stored into the
    heads) -> D2H of the header region only -> rns_io_send_batch_chain (each datagram
    gathered from [head, payload], as send_packet's to_iovec + writev send a NetBuffer,
    netif.rs:51-98)."""

    HEAD_MAX = 128  # bytes per head fragment, at most (IPv4 with options + TCP with options)
    DEPTH = 2

    def __init__(self, device: int = 0, max_pkts: int = 65536, payload_bytes: int | None = None,
                 compact: bool = False):
        self.max_pkts = max_pkts
        # compact=True: a batch whose payloads are exactly packed (chain_compact_form) sends only the
        # compact descriptors to the device (3 B per datagram + 16 B per 64, not 28 B) and is finalized
        # by rns_tx_fill_chain_packed_dev; any other batch takes the CSR route.  last_form / last_desc_bytes:
        # the route of the last batch queued ("compact" or "csr") and the descriptor bytes it copied H2D.
        self.compact = compact
        self.last_form: str | None = None
        self.last_desc_bytes = 0
        self.dev = torch.device(f"cuda:{device}")
        self.head_region = (self.HEAD_MAX * max_pkts + 4095) & ~4095
        self.payload_bytes = payload_bytes if payload_bytes is not None else MRU * max_pkts
        self._sets = [_ChainSet(self.dev, max_pkts, self.head_region, self.payload_bytes, compact)
                      for _ in range(self.DEPTH)]
        self._next = 0
        self._inflight: deque = deque()
        self._stream = None

    def heads(self) -> np.ndarray:
        """The free set's header region: head fragments back to back in datagram order."""
        if len(self._inflight) == self.DEPTH:
            raise RuntimeError("every buffer set is in flight: complete() one first")
        return self._sets[self._next].host.array[: self.head_region]

    def payloads(self) -> np.ndarray:
        """The free set's payload region (offsets passed to send / submit are relative to it)."""
        if len(self._inflight) == self.DEPTH:
            raise RuntimeError("every buffer set is in flight: complete() one first")
        return self._sets[self._next].host.array[self.head_region: self.head_region + self.payload_bytes]

    def pending(self) -> int:
        return len(self._inflight)

    def _describe(self, s: _ChainSet, head_len, pay_off, pay_len):
        """Chain descriptors [head, payload (if any)] per datagram into the set's pinned arrays;
        returns (n, fragments, header bytes used, payload bytes used)."""
        hl = np.ascontiguousarray(head_len, dtype=np.int64)
        po = np.ascontiguousarray(pay_off, dtype=np.int64)
        pl = np.ascontiguousarray(pay_len, dtype=np.int64)
        n = hl.shape[0]
        if po.shape[0] != n or pl.shape[0] != n:
            raise ValueError("head_len, pay_off and pay_len need one entry per datagram")
        if n > self.max_pkts:
            raise ValueError("more datagrams than the pipeline holds")
        if n and (hl.min() < 1 or hl.max() > self.HEAD_MAX or pl.min() < 0 or po.min() < 0 or
                  int((po + pl).max()) > self.payload_bytes):
            raise ValueError(f"head lengths must be 1..{self.HEAD_MAX} and payloads inside payloads()")
        hoff = np.zeros(n, dtype=np.int64)
        if n > 1:
            np.cumsum(hl[:-1], out=hoff[1:])
        nfr = 1 + (pl > 0)
        first = s.h_first.array.view(np.uint32)[: n + 1]
        first[0] = 0
        first[1:] = np.cumsum(nfr)
        nf = int(first[n])
        off = s.h_off.array.view(np.uint64)[:nf]
        ln = s.h_len.array.view(np.uint32)[:nf]
        f0 = first[:n].astype(np.int64)
        off[f0] = hoff.astype(np.uint64)
        ln[f0] = hl.astype(np.uint32)
        has = pl > 0
        off[f0[has] + 1] = (po[has] + self.head_region).astype(np.uint64)
        ln[f0[has] + 1] = pl[has].astype(np.uint32)
        hused = int(hoff[-1] + hl[-1]) if n else 0
        pused = int((po + pl).max()) if n else 0
        # the compact route (its descriptors into the set's pinned buffer), when the batch has that form
        s.cform = False
        if self.compact and n:
            c = chain_compact_form(hl, po, pl, self.head_region)
            if c is not None:
                nb = (n + 63) // 64
                h = s.h_cdesc.array
                h[:8 * nb].view(np.uint64)[:] = c[0]
                h[8 * nb:16 * nb].view(np.uint64)[:] = c[2]
                h[16 * nb:16 * nb + 2 * n].view(np.uint16)[:] = c[3]
                h[16 * nb + 2 * n:16 * nb + 3 * n] = c[1]
                s.cform = True
        return n, nf, hused, pused

    def _queue(self, s: _ChainSet, n: int, nf: int, hused: int, pused: int) -> None:
        hr = self.head_region
        s.d_arena[:hused].copy_(torch.from_numpy(s.host.array[:hused]), non_blocking=True)
        if pused:
            s.d_arena[hr:hr + pused].copy_(torch.from_numpy(s.host.array[hr:hr + pused]), non_blocking=True)
        if s.cform:
            nb, cb = (n + 63) // 64, compact_desc_bytes(n)
            d = s.d_cdesc
            d[:cb].copy_(torch.from_numpy(s.h_cdesc.array[:cb]), non_blocking=True)
            tx_fill_chain_packed(s.d_arena, d[:8 * nb].view(torch.int64), d[16 * nb + 2 * n:cb],
                                 d[8 * nb:16 * nb].view(torch.int64), d[16 * nb:16 * nb + 2 * n].view(torch.uint16),
                                 pay_align_log2=4, status=s.d_status[:n])
            self.last_form, self.last_desc_bytes = "compact", cb
        else:
            s.d_off[:nf].copy_(torch.from_numpy(s.h_off.array.view(np.int64)[:nf]), non_blocking=True)
            s.d_len[:nf].copy_(torch.from_numpy(s.h_len.array.view(np.int32)[:nf]), non_blocking=True)
            s.d_first[:n + 1].copy_(torch.from_numpy(s.h_first.array.view(np.int32)[:n + 1]), non_blocking=True)
            tx_fill_chain(s.d_arena, s.d_off[:nf], s.d_len[:nf], s.d_first[:n + 1], status=s.d_status[:n])
            self.last_form, self.last_desc_bytes = "csr", 12 * nf + 4 * (n + 1)
        torch.from_numpy(s.host.array[:hused]).copy_(s.d_arena[:hused], non_blocking=True)
        torch.from_numpy(s.h_status.array[:n]).copy_(s.d_status[:n], non_blocking=True)
        s.done.record()

    def _finish(self, fd: int, s: _ChainSet, n: int, nf: int) -> np.ndarray:
        s.done.synchronize()
        sent = send_batch_chain(fd, s.host.array, s.h_off.array.view(np.uint64)[:nf],
                                s.h_len.array.view(np.uint32)[:nf], s.h_first.array.view(np.uint32)[:n + 1])
        if sent != n:
            raise OSError(f"sent {sent} of {n} datagrams")
        return s.h_status.array[:n].copy()

    def send(self, fd: int, head_len, pay_off, pay_len) -> np.ndarray:
        """Finalize and send datagrams [0, n) of ``heads()`` / ``payloads()``; returns their
        RNS_TX_* status."""
        if self._inflight:
            raise RuntimeError("submitted batches pending: complete() them first")
        s = self._sets[self._next]
        n, nf, hused, pused = self._describe(s, head_len, pay_off, pay_len)
        if n == 0:
            return np.empty(0, dtype=np.uint8)
        with torch.cuda.device(self.dev):
            self._queue(s, n, nf, hused, pused)
        return self._finish(fd, s, n, nf)

    def submit(self, head_len, pay_off, pay_len) -> None:
        """Queue the GPU work for the free set's datagrams and hand out the other set."""
        if len(self._inflight) == self.DEPTH:
            raise RuntimeError("every buffer set is in flight: complete() one first")
        s = self._sets[self._next]
        n, nf, hused, pused = self._describe(s, head_len, pay_off, pay_len)
        with torch.cuda.device(self.dev):
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.dev)
            with torch.cuda.stream(self._stream):
                if n:
                    self._queue(s, n, nf, hused, pused)
                else:
                    s.done.record()
        self._inflight.append((s, n, nf))
        self._next = (self._next + 1) % self.DEPTH

    def complete(self, fd: int) -> np.ndarray:
        """Wait for the oldest submitted batch, send it; returns its RNS_TX_* status."""
        if not self._inflight:
            raise RuntimeError("nothing submitted")
        s, n, nf = self._inflight.popleft()
        if n == 0:
            return np.empty(0, dtype=np.uint8)
        return self._finish(fd, s, n, nf)

    def close(self):
        for s in self._sets:
            s.close()


class PoolChains:
    """The datagrams of one RxPoolPipeline batch: ``c[i]`` = (buffer indices uint32, length) of
    datagram i, ``c.bytes(i)`` its bytes gathered from the host pool (valid while its buffers are
    held)."""

    def __init__(self, pool: np.ndarray, buf_bytes: int, idx: np.ndarray, first: np.ndarray, length: np.ndarray):
        self.pool, self.buf_bytes, self.idx, self.first, self.length = pool, buf_bytes, idx, first, length

    def __len__(self) -> int:
        return int(self.length.shape[0])

    def __getitem__(self, i: int) -> tuple[np.ndarray, int]:
        return self.idx[int(self.first[i]):int(self.first[i + 1])], int(self.length[i])

    def bytes(self, i: int) -> bytes:
        idx, n = self[i]
        rows = self.pool.reshape(-1, self.buf_bytes)[idx]
        return rows.tobytes()[:n]


class RxPoolPipeline:
    """Batched receive into a buffer pool and verify in place: datagram fd -> pinned pool of
    ``pool_bufs`` buffers of ``buf_bytes`` (recv_packet's NetBuffer chains, netif.rs:65-83) -> the
    same offsets of a device mirror -> rns_rx_verify_pool_dev.  Buffers a batch used stay held, as a
    TCP reassembly queue holds them, until ``release`` returns them to the free list; the next
    batch takes free buffers only.  ``h2d_bytes``: the pool bytes the last ``receive`` copied (the
    covering span of the buffers it used), ``desc_bytes``: its descriptor bytes."""

    def __init__(self, local_ipv4: bytes, local_ipv6: bytes, device: int = 0, pool_bufs: int | None = None,
                 buf_bytes: int = 512, mru: int = MRU, max_pkts: int = 65536):
        self.local_ipv4, self.local_ipv6 = bytes(local_ipv4), bytes(local_ipv6)
        self.buf_bytes, self.mru, self.max_pkts = int(buf_bytes), int(mru), int(max_pkts)
        need = -(-self.mru // self.buf_bytes)
        self.pool_bufs = int(pool_bufs) if pool_bufs is not None else self.max_pkts * need
        self.dev = torch.device(f"cuda:{device}")
        nblk = (self.max_pkts + 63) // 64
        self.host = PinnedBuffer(self.pool_bufs * self.buf_bytes)
        self._h_idx, self._h_len = PinnedBuffer(4 * self.pool_bufs), PinnedBuffer(2 * self.max_pkts)
        self._h_blk, self._h_status = PinnedBuffer(4 * nblk), PinnedBuffer(self.max_pkts)
        self._h_l4 = PinnedBuffer(2 * self.max_pkts)
        self.d_pool = torch.empty(self.pool_bufs * self.buf_bytes, dtype=torch.uint8, device=self.dev)
        self._d_idx = torch.empty(self.pool_bufs, dtype=torch.int32, device=self.dev)
        self._d_len = torch.empty(self.max_pkts, dtype=torch.int16, device=self.dev)
        self._d_blk = torch.empty(nblk, dtype=torch.int32, device=self.dev)
        self._d_status = torch.empty(self.max_pkts, dtype=torch.uint8, device=self.dev)
        self._d_l4 = torch.empty(self.max_pkts, dtype=torch.int16, device=self.dev)
        self._done = torch.cuda.Event()
        self._free = np.arange(self.pool_bufs, dtype=np.uint32)
        self._held = np.zeros(self.pool_bufs, dtype=bool)
        self.h2d_bytes = 0
        self.desc_bytes = 0

    @property
    def free_bufs(self) -> int:
        return int(self._free.shape[0])

    def receive(self, fd: int, timeout_ms: int = 0) -> tuple[np.ndarray, np.ndarray, PoolChains]:
        """One batch: (status uint8 [n], l4_sum uint16 [n], chains)."""
        free = self._free
        n, len16, blk, nf = recv_batch_pool(fd, self.host.array, free, self.buf_bytes, self.mru, self.max_pkts,
                                            timeout_ms)
        self.h2d_bytes = self.desc_bytes = 0
        idx = free[:nf].copy()
        first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(-(-len16.astype(np.int64) // self.buf_bytes), out=first[1:])
        chains = PoolChains(self.host.array, self.buf_bytes, idx, first, len16.copy())
        if n == 0:
            return np.empty(0, dtype=np.uint8), np.empty(0, dtype=np.uint16), chains
        self._free = free[nf:].copy()
        self._held[idx] = True
        nb = blk.shape[0]
        h_idx, h_len = self._h_idx.array.view(np.int32)[:nf], self._h_len.array.view(np.int16)[:n]
        h_blk = self._h_blk.array.view(np.int32)[:nb]
        h_idx[:], h_len[:], h_blk[:] = idx.view(np.int32), len16.view(np.int16), blk.view(np.int32)
        lo, hi = int(idx.min()) * self.buf_bytes, (int(idx.max()) + 1) * self.buf_bytes
        with torch.cuda.device(self.dev):
            # pinned host memory (rns_host_alloc): every copy is a DMA transfer
            self.d_pool[lo:hi].copy_(torch.from_numpy(self.host.array[lo:hi]), non_blocking=True)
            self._d_idx[:nf].copy_(torch.from_numpy(h_idx), non_blocking=True)
            self._d_len[:n].copy_(torch.from_numpy(h_len), non_blocking=True)
            self._d_blk[:nb].copy_(torch.from_numpy(h_blk), non_blocking=True)
            self.h2d_bytes, self.desc_bytes = hi - lo, 4 * nf + 2 * n + 4 * nb
            rx_verify_pool(self.d_pool, self._d_idx[:nf], self._d_blk[:nb], self._d_len[:n], self.local_ipv4,
                           self.local_ipv6, buf_bytes=self.buf_bytes, status=self._d_status[:n],
                           l4_sum=self._d_l4[:n])
            torch.from_numpy(self._h_status.array[:n]).copy_(self._d_status[:n], non_blocking=True)
            torch.from_numpy(self._h_l4.array.view(np.int16)[:n]).copy_(self._d_l4[:n], non_blocking=True)
            self._done.record()
            self._done.synchronize()
        return self._h_status.array[:n].copy(), self._h_l4.array.view(np.uint16)[:n].copy(), chains

    def release(self, indices) -> None:
        """Return held buffers to the free list (each index once, and only while it is held).  The list
        is kept in index order: the next batch takes the lowest free buffers, so the span it copies
        stays close to the buffers it uses instead of wrapping round the pool."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
        if idx.size == 0:
            return
        if int(idx.max()) >= self.pool_bufs or not self._held[idx].all() or np.unique(idx).size != idx.size:
            raise ValueError("release takes indices of held buffers, each once")
        self._held[idx] = False
        self._free = np.sort(np.concatenate([self._free, idx]))

    def close(self):
        for b in (self.host, self._h_idx, self._h_len, self._h_blk, self._h_status, self._h_l4):
            b.free()


class TxPoolPipeline:
    """Batched transmit out of a buffer pool: pinned pool of ``pool_bufs`` buffers of ``buf_bytes``
    (the reference's NetBuffer pool: alloc_header's head buffer with its data at the end, buf.rs:262-291,
    then append_from_slice's payload buffers, buf.rs:385-420) -> the same offsets of a device mirror ->
    rns_tx_fill_pool_dev -> the heads' tails back -> datagram fd.  ``alloc`` hands out free buffers
    and marks them held; they stay held, as a TCP retransmit queue holds them, until ``release``
    returns them.  ``h2d_bytes``: the pool bytes the last ``send`` copied (the covering span of the
    buffers it used), ``d2h_bytes``: the head bytes it brought back, ``desc_bytes``: its descriptor
    bytes (3 B per datagram + 4 B per buffer + 4 B per 64 datagrams)."""

    def __init__(self, device: int = 0, pool_bufs: int | None = None, max_pkts: int = 8192, buf_bytes: int = 512):
        self.buf_bytes, self.max_pkts = int(buf_bytes), int(max_pkts)
        _buf_log2(self.buf_bytes, 256)
        self.pool_bufs = int(pool_bufs) if pool_bufs is not None else self.max_pkts * (1 + -(-MRU // self.buf_bytes))
        self.tail = min(self.buf_bytes, 256)  # the bytes of a head buffer a head (<= 255) can lie in
        self.dev = torch.device(f"cuda:{device}")
        nblk = (self.max_pkts + 63) // 64
        self.host = PinnedBuffer(self.pool_bufs * self.buf_bytes)
        self._h_idx, self._h_hl = PinnedBuffer(4 * self.pool_bufs), PinnedBuffer(self.max_pkts)
        self._h_pl, self._h_blk = PinnedBuffer(2 * self.max_pkts), PinnedBuffer(4 * nblk)
        self._h_status, self._h_heads = PinnedBuffer(self.max_pkts), PinnedBuffer(self.max_pkts * self.tail)
        self.d_pool = torch.empty(self.pool_bufs * self.buf_bytes, dtype=torch.uint8, device=self.dev)
        self._d_idx = torch.empty(self.pool_bufs, dtype=torch.int32, device=self.dev)
        self._d_hl = torch.empty(self.max_pkts, dtype=torch.uint8, device=self.dev)
        self._d_pl = torch.empty(self.max_pkts, dtype=torch.int16, device=self.dev)
        self._d_blk = torch.empty(nblk, dtype=torch.int32, device=self.dev)
        self._d_status = torch.empty(self.max_pkts, dtype=torch.uint8, device=self.dev)
        self._d_heads = torch.empty(self.max_pkts, self.tail, dtype=torch.uint8, device=self.dev)
        self._done = torch.cuda.Event()
        self._free = np.arange(self.pool_bufs, dtype=np.uint32)
        self._held = np.zeros(self.pool_bufs, dtype=bool)
        self.h2d_bytes = self.d2h_bytes = self.desc_bytes = 0

    @property
    def free_bufs(self) -> int:
        return int(self._free.shape[0])

    def _lengths(self, head_len, pay_len) -> tuple[np.ndarray, np.ndarray]:
        hl, pl = np.asarray(head_len), np.asarray(pay_len)
        if hl.ndim != 1 or hl.shape != pl.shape or hl.shape[0] > self.max_pkts:
            raise ValueError(f"head_len and pay_len: one entry per datagram each, at most {self.max_pkts}")
        if hl.size and not (1 <= int(hl.min()) and int(hl.max()) <= 255 and 0 <= int(pl.min()) and int(pl.max()) <= 0xFFFF):
            raise ValueError("head lengths are 1..255 and payload lengths 0..65535")
        return hl.astype(np.uint8), pl.astype(np.uint16)

    def alloc(self, head_len, pay_len) -> np.ndarray:
        """The buffer indices (uint32, in the form's order: each datagram's head buffer, then its
        payload buffers) of a batch with these lengths, taken from the free list and marked held."""
        _, pl = self._lengths(head_len, pay_len)
        nf = int((1 + -(-pl.astype(np.int64) // self.buf_bytes)).sum())
        if nf > self._free.shape[0]:
            raise ValueError(f"the batch needs {nf} buffers, {self._free.shape[0]} are free")
        idx, self._free = self._free[:nf].copy(), self._free[nf:].copy()
        self._held[idx] = True
        return idx

    def send(self, fd: int, buf_idx, head_len, pay_len) -> np.ndarray:
        """Finalize and send one batch whose heads (at each head buffer's end) and payloads the caller
        wrote into ``host``; returns the uint8 status (RNS_TX_*) per datagram."""
        hl, pl = self._lengths(head_len, pay_len)
        idx = np.ascontiguousarray(buf_idx, dtype=np.uint32).ravel()
        n = int(hl.shape[0])
        self.h2d_bytes = self.d2h_bytes = self.desc_bytes = 0
        if n == 0:
            return np.empty(0, dtype=np.uint8)
        blk, first, nf = tx_pool_layout(pl, self.buf_bytes)
        if idx.shape[0] != nf or int(idx.max()) >= self.pool_bufs or not self._held[idx].all():
            raise ValueError("buf_idx must name the batch's held buffers, one per fragment")
        heads = idx[first[:-1]].astype(np.int64)
        if np.unique(heads).size != n:
            raise ValueError("a head buffer is named twice")
        nb, B, tail = blk.shape[0], self.buf_bytes, self.tail
        h_idx, h_blk = self._h_idx.array.view(np.int32)[:nf], self._h_blk.array.view(np.int32)[:nb]
        h_hl, h_pl = self._h_hl.array[:n], self._h_pl.array.view(np.int16)[:n]
        h_idx[:], h_blk[:], h_hl[:], h_pl[:] = idx.view(np.int32), blk.view(np.int32), hl, pl.view(np.int16)
        lo, hi = int(idx.min()) * B, (int(idx.max()) + 1) * B
        h_heads = self._h_heads.array[:n * tail].reshape(n, tail)
        with torch.cuda.device(self.dev):
            # pinned host memory (rns_host_alloc): every copy is a DMA transfer
            self.d_pool[lo:hi].copy_(torch.from_numpy(self.host.array[lo:hi]), non_blocking=True)
            self._d_idx[:nf].copy_(torch.from_numpy(h_idx), non_blocking=True)
            self._d_blk[:nb].copy_(torch.from_numpy(h_blk), non_blocking=True)
            self._d_hl[:n].copy_(torch.from_numpy(h_hl), non_blocking=True)
            self._d_pl[:n].copy_(torch.from_numpy(h_pl), non_blocking=True)
            self.h2d_bytes, self.desc_bytes = hi - lo, 3 * n + 4 * nf + 4 * nb
            tx_fill_pool(self.d_pool, self._d_idx[:nf], self._d_blk[:nb], self._d_hl[:n], self._d_pl[:n],
                         buf_bytes=B, status=self._d_status[:n])
            # only the heads come back: the last `tail` bytes of every head buffer gathered on the device
            # (the head buffers' places in buf_idx follow from the payload lengths already there)
            nfr = 1 + ((self._d_pl[:n].to(torch.int64) & 0xFFFF) + (B - 1)) // B
            d_heads = self._d_idx[:nf][torch.cumsum(nfr, 0) - nfr].to(torch.int64)
            torch.index_select(self.d_pool.view(self.pool_bufs, B)[:, B - tail:], 0, d_heads, out=self._d_heads[:n])
            torch.from_numpy(h_heads).copy_(self._d_heads[:n], non_blocking=True)
            torch.from_numpy(self._h_status.array[:n]).copy_(self._d_status[:n], non_blocking=True)
            self.d2h_bytes = n * tail
            self._done.record()
            self._done.synchronize()
        self.host.array.reshape(self.pool_bufs, B)[heads, B - tail:] = h_heads
        sent = send_batch_pool(fd, self.host.array, idx, blk, hl, pl, B)
        if sent != n:
            raise RuntimeError(f"sent {sent} of {n} datagrams")
        return self._h_status.array[:n].copy()

    def release(self, indices) -> None:
        """Return held buffers to the free list (each index once, and only while it is held); the list
        is kept in index order, as RxPoolPipeline keeps it."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
        if idx.size == 0:
            return
        if int(idx.max()) >= self.pool_bufs or not self._held[idx].all() or np.unique(idx).size != idx.size:
            raise ValueError("release takes indices of held buffers, each once")
        self._held[idx] = False
        self._free = np.sort(np.concatenate([self._free, idx]))

    def close(self):
        for b in (self.host, self._h_idx, self._h_hl, self._h_pl, self._h_blk, self._h_status, self._h_heads):
            b.free()


class TxSegmentPipeline:
    """Bulk TCP sends with the segment loop on the device (tcp_write, tcp.rs:256-285): the caller
    writes each send's data into the pinned payload region ``host.array[:pay_bytes]`` (any byte
    alignment) and passes one template head, the data's offset and length and the mss per send.
    Data, templates and per-send descriptors go up; rns_tx_segment_dev builds and finalizes every
    segment's head in the header region behind the payload region; only that region comes back, and
    the [head, data slice] chains go out on the datagram fd (rns_io_send_batch_chain).  ``send`` is
    synchronous.  ``h2d_bytes``: the payload span, templates and descriptors the last ``send``
    copied up, ``desc_bytes``: the descriptors' share of that (27 B per send + 4 B per 64 segments),
    ``d2h_bytes``: the head bytes it brought back."""

    def __init__(self, device: int = 0, pay_bytes: int = 16 << 20, max_flows: int = 1024, max_segs: int = 16384,
                 tmpl_stride: int = 100):
        self.pay_bytes = (int(pay_bytes) + 15) // 16 * 16
        self.max_flows, self.max_segs, self.stride = int(max_flows), int(max_segs), int(tmpl_stride)
        if not 40 <= self.stride <= 255:
            raise ValueError("tmpl_stride must be in 40..255")
        self.hdr_bytes = self.max_segs * self.stride
        self.dev = torch.device(f"cuda:{device}")
        self.host = PinnedBuffer(self.pay_bytes + self.hdr_bytes)
        # per-send descriptors, one pinned block: templates, then the u64 / u32 / u16 / u8 arrays
        nf, nb = self.max_flows, (self.max_segs + 63) // 64
        self._lay = []
        at = 0
        for name, dt, cnt in (("tmpl", np.uint8, nf * self.stride), ("po", np.int64, nf), ("ho", np.int64, nf),
                              ("pl", np.int32, nf), ("sf", np.int32, nf + 1), ("bf", np.int32, nb),
                              ("mss", np.int16, nf), ("hl", np.uint8, nf)):
            at = (at + 15) // 16 * 16
            self._lay.append((name, np.dtype(dt), at, cnt))
            at += np.dtype(dt).itemsize * cnt
        self._h_desc, self._h_status = PinnedBuffer(at), PinnedBuffer(self.max_segs)
        self.d_arena = torch.empty(self.pay_bytes + self.hdr_bytes, dtype=torch.uint8, device=self.dev)
        self._d_desc = torch.empty(at, dtype=torch.uint8, device=self.dev)
        self._d_status = torch.empty(self.max_segs, dtype=torch.uint8, device=self.dev)
        self._done = torch.cuda.Event()
        self.h2d_bytes = self.d2h_bytes = self.desc_bytes = 0

    def send(self, fd: int, templates, pay_off, pay_len, mss) -> np.ndarray:
        """Segment, finalize and send the given sends; returns the uint8 status (RNS_TX_*) per
        segment, in send order.  Nothing is sent unless every segment is well formed."""
        tm = [bytes(t) for t in templates]
        nfl = len(tm)
        po, pl = np.asarray(pay_off, dtype=np.uint64), np.asarray(pay_len, dtype=np.uint32)
        ms = np.asarray(mss, dtype=np.uint16)
        self.h2d_bytes = self.d2h_bytes = self.desc_bytes = 0
        if nfl == 0:
            return np.empty(0, dtype=np.uint8)
        if nfl > self.max_flows or po.shape != (nfl,) or pl.shape != (nfl,) or ms.shape != (nfl,):
            raise ValueError(f"one template, offset, length and mss per send, at most {self.max_flows} sends")
        if max(len(t) for t in tm) > self.stride or min(len(t) for t in tm) < 40:
            raise ValueError(f"template heads are 40..{self.stride} bytes")
        if int((po + pl).max()) > self.pay_bytes:
            raise ValueError("a send's data lies outside the payload region")
        hl = np.array([len(t) for t in tm], dtype=np.uint8)
        seg_first, head_off, blk_flow, n_seg, head_end = tx_segment_layout(pl, ms, hl, self.pay_bytes)
        if n_seg > self.max_segs or head_end > self.pay_bytes + self.hdr_bytes:
            raise ValueError(f"the sends make {n_seg} segments; the pipeline holds {self.max_segs}")
        if n_seg == 0:
            return np.empty(0, dtype=np.uint8)
        nb = blk_flow.shape[0]
        vals = {"po": po.view(np.int64), "ho": head_off.view(np.int64), "pl": pl.view(np.int32),
                "sf": seg_first.view(np.int32), "bf": blk_flow.view(np.int32), "mss": ms.view(np.int16), "hl": hl}
        h, d, used = {}, {}, 0
        for name, dt, at, cnt in self._lay:
            h[name] = self._h_desc.array[at:at + dt.itemsize * cnt].view(dt)
            d[name] = self._d_desc[at:at + dt.itemsize * cnt].view(getattr(torch, dt.name))
            k = nfl * self.stride if name == "tmpl" else vals[name].shape[0]
            if name == "tmpl":
                rows = h[name][:k].reshape(nfl, self.stride)
                for i, t in enumerate(tm):
                    rows[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
            else:
                h[name][:k] = vals[name]
            used = max(used, at + dt.itemsize * k)
        nz = pl > 0
        lo = int(po[nz].min()) & ~15
        hi = int((po + pl)[nz].max())
        with torch.cuda.device(self.dev):
            # pinned host memory (rns_host_alloc): every copy is a DMA transfer
            self.d_arena[lo:hi].copy_(torch.from_numpy(self.host.array[lo:hi]), non_blocking=True)
            self._d_desc[:used].copy_(torch.from_numpy(self._h_desc.array[:used]), non_blocking=True)
            self.desc_bytes = 27 * nfl + 4 * nb
            self.h2d_bytes = hi - lo + nfl * self.stride + self.desc_bytes
            tx_segment(self.d_arena, d["tmpl"][:nfl * self.stride].view(nfl, self.stride), d["hl"][:nfl], d["po"][:nfl],
                       d["pl"][:nfl], d["mss"][:nfl], d["ho"][:nfl], d["sf"][:nfl + 1], d["bf"][:nb], n_seg,
                       status=self._d_status[:n_seg])
            # only the header region comes back
            torch.from_numpy(self.host.array[self.pay_bytes:head_end]).copy_(self.d_arena[self.pay_bytes:head_end],
                                                                             non_blocking=True)
            torch.from_numpy(self._h_status.array[:n_seg]).copy_(self._d_status[:n_seg], non_blocking=True)
            self.d2h_bytes = head_end - self.pay_bytes
            self._done.record()
            self._done.synchronize()
        status = self._h_status.array[:n_seg].copy()
        if (status & 0x80).any():
            return status
        frag_off, frag_len, first = tx_segment_chains(po, pl, ms, hl, head_off)
        sent = send_batch_chain(fd, self.host.array, frag_off, frag_len, first)
        if sent != n_seg:
            raise RuntimeError(f"sent {sent} of {n_seg} datagrams")
        return status

    def close(self):
        for b in (self.host, self._h_desc, self._h_status):
            b.free()
