"""TCP receive placement: tcp_input's decode, the PORT_MAP lookup and tcp_read's copy on the device.

After validate_checksum, tcp_input (tcp.rs:549-652) decodes the TCP header, looks the socket up by
``(source_ip, source_port, dest_port)`` and hands the payload to the reassembler; tcp_read later
copies it out of 512-byte fragments.  ``rx_tcp_place_pool`` does all of it for a batch held in the
pool form (``pool.rx_verify_pool``'s layout): every accepted segment is decoded into a 24-byte
record (``META_DTYPE``), its flow found in a table built by ``rx_flow_table``, and its payload
copied to ``window start + (seq - next expected seq)`` of that flow's contiguous receive window
(rns_rx_tcp_place_pool_dev).  ``Reassembler`` is the reference's TCPReassembler over (seq, length)
pairs with the data already in place: it says how far a flow's window has become readable.  The
functions are re-exported by ``batch``, whose argument checks they use.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .batch import _I32, _I64, _U8, _call, _local_addrs, _nonnull, _per_packet, _seq_gt, _status
from .pool import _pool_batch

# rns_rx_tcp_meta (rns_checksum.h), one record per datagram
META_DTYPE = np.dtype([("flow", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                       ("window", "<u2"), ("pay_len", "<u2"), ("flags", "u1"), ("ip_hdr", "u1"), ("tcp_hdr", "u1"),
                       ("place", "u1")])
assert META_DTYPE.itemsize == 24
# rns_rx_flow_key
KEY_DTYPE = np.dtype([("ip", "u1", (16,)), ("sport", "<u2"), ("dport", "<u2"), ("family", "u1"), ("pad", "u1", (3,))])
assert KEY_DTYPE.itemsize == 24


def _keys(keys) -> np.ndarray:
    """``keys``: a KEY_DTYPE array, or an iterable of ``(remote ip bytes (4 or 16), sport, dport)``."""
    if isinstance(keys, np.ndarray) and keys.dtype == KEY_DTYPE:
        return np.ascontiguousarray(keys).reshape(-1)
    keys = list(keys)
    arr = np.zeros(len(keys), dtype=KEY_DTYPE)
    for f, (ip, sport, dport) in enumerate(keys):
        ip = bytes(ip)
        if len(ip) not in (4, 16):
            raise ValueError("a flow key's address must be 4 or 16 bytes")
        if not (0 <= int(sport) <= 0xFFFF and 0 <= int(dport) <= 0xFFFF):
            raise ValueError("ports are u16")
        arr["ip"][f, :len(ip)] = np.frombuffer(ip, dtype=np.uint8)
        arr["sport"][f], arr["dport"][f], arr["family"][f] = int(sport), int(dport), 4 if len(ip) == 4 else 6
    return arr


def rx_flow_table(keys) -> np.ndarray:
    """The placement's flow table (rns_rx_flow_table_build) for PORT_MAP's keys (tcp.rs:578: the
    remote address, the remote port, the local port), key f mapped to flow index f: a uint8 array to
    copy to the device as it is.  A duplicate key is refused."""
    arr = _keys(keys)
    n = int(arr.size)
    if n >= 2 ** 31:
        raise ValueError("at most 2^31-1 flows")
    need = ctypes.c_uint64(0)
    lib = _lib.load()
    _lib.check(lib.rns_rx_flow_table_build(arr.ctypes.data, n, None, 0, ctypes.byref(need)), "rns_rx_flow_table_build")
    tbl = np.zeros(int(need.value), dtype=np.uint8)
    _lib.check(lib.rns_rx_flow_table_build(arr.ctypes.data, n, tbl.ctypes.data, tbl.size, ctypes.byref(need)),
               "rns_rx_flow_table_build")
    return tbl


def meta_records(meta: torch.Tensor) -> np.ndarray:
    """The device's meta bytes as a numpy array of META_DTYPE records (a copy on the host)."""
    return meta.detach().cpu().contiguous().numpy().reshape(-1).view(META_DTYPE)


def rx_tcp_place_pool(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor,
                      local_ipv4: bytes, local_ipv6: bytes, table: torch.Tensor, next_seq: torch.Tensor,
                      win_off: torch.Tensor, win_len: torch.Tensor, stream: torch.Tensor, *, buf_bytes: int = 512,
                      status: torch.Tensor | None = None, l4_sum: torch.Tensor | None = None,
                      meta: torch.Tensor | None = None):
    """TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev).  ``pool`` / ``buf_idx`` /
    ``blk_first`` / ``len16`` as for ``rx_verify_pool`` (``buf_bytes`` a power of two in 128..32768),
    ``table`` = ``rx_flow_table``'s bytes on the device, flow f's window =
    ``stream[win_off[f] : win_off[f] + win_len[f]]`` whose first byte has sequence number
    ``next_seq[f]`` (int32 tensors hold the u32 values).  Every accepted TCP segment is decoded into
    ``meta[i]`` (a uint8 tensor of n x 24 bytes: ``meta_records`` gives META_DTYPE records) and, when
    its flow is in the table and its payload lies inside the window, the payload is copied to
    ``win_off[f] + (seq - next_seq[f])``.  Returns ``(status, l4_sum, meta)``; status and l4_sum are
    ``rx_verify_pool``'s."""
    dev, log2, n, nf = _pool_batch(pool, buf_idx, blk_first, len16, buf_bytes, 128, ("table", table, _U8),
                                   ("next_seq", next_seq, _I32), ("win_off", win_off, _I64), ("win_len", win_len, _I32),
                                   ("stream", stream, _U8))
    nfl = next_seq.numel()
    if win_off.numel() != nfl or win_len.numel() != nfl:
        raise ValueError("next_seq, win_off and win_len need one entry per flow each")
    if pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    if meta is None:
        meta = torch.empty((n, META_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _per_packet(meta, "meta", n * META_DTYPE.itemsize, dev, _U8)
    ptr = _nonnull(dev)
    _call("rns_rx_tcp_place_pool_dev", dev, pool.data_ptr(), pool.numel(), log2, buf_idx.data_ptr(), nf,
          blk_first.data_ptr(), len16.data_ptr(), n, ip4, ip6, table.data_ptr(), table.numel(), ptr(next_seq),
          ptr(win_off), ptr(win_len), nfl, ptr(stream), stream.numel(), status.data_ptr(),
          _per_packet(l4_sum, "l4_sum", n, dev), meta.data_ptr())
    return status, l4_sum, meta


class Reassembler:
    """TCPReassembler (tcp.rs:476-521) over ``(seq, length)`` pairs, the data already in place: the
    same pending list, the same removal rule (seq_gt against the ARRIVING segment's seq) and the same
    rescan, so ``get_next_expect()`` equals the reference's after every call, overlaps included."""

    def __init__(self, next_expect: int = 0):
        self.next_sequence = int(next_expect) & 0xFFFFFFFF
        self.out_of_order: list[tuple[int, int]] = []

    def set_next_expect(self, seq: int) -> None:
        self.next_sequence = int(seq) & 0xFFFFFFFF

    def get_next_expect(self) -> int:
        return self.next_sequence

    def add(self, seq: int, length: int) -> int:
        """add_packet: the bytes that became readable (the reference's returned buffer's length), 0
        if the segment is out of order (it is then pending)."""
        seq, length = int(seq) & 0xFFFFFFFF, int(length)
        if seq != self.next_sequence:
            self.out_of_order.append((seq, length))
            return 0
        got = length
        self.next_sequence = (self.next_sequence + length) & 0xFFFFFFFF
        i = 0
        while i < len(self.out_of_order):
            if _seq_gt(seq, self.out_of_order[i][0]):
                del self.out_of_order[i]
            elif self.out_of_order[i][0] == self.next_sequence:
                _, ln = self.out_of_order.pop(i)
                self.next_sequence = (self.next_sequence + ln) & 0xFFFFFFFF
                got += ln
                i = 0
            else:
                i += 1
        return got

    def feed(self, meta: np.ndarray, flow: int) -> int:
        """Add flow ``flow``'s placed segments (RNS_PLACE_DONE) of one batch's META_DTYPE records, in
        batch order; returns the bytes that became readable."""
        m = np.asarray(meta).reshape(-1)
        sel = m[(m["flow"] == flow) & ((m["place"] & _lib.RNS_PLACE_DONE) != 0)]
        return sum(self.add(int(r["seq"]), int(r["pay_len"])) for r in sel)
