"""MI355X-native batched Internet checksum — the hot path of jbush001/RustNetworkStack
(src/stack/util.rs:86-119, 180-207), as hand-written gfx950 HIP kernels behind a C ABI
(include/rns_checksum.h).

* ``util``      — the reference's `netstack::util` checksum surface, same names and errors;
* ``batch``     — device-resident / host-resident batch API (torch tensors, numpy arrays);
* ``pool``      — receive verify and transmit finalize of datagrams in pool buffers over compact
                  descriptors (also ``batch.*``);
* ``segment``   — TCP segmentation offload: one template head per send, the segments' heads built
                  and finalized on the device (also ``batch.*``);
* ``place``     — TCP receive placement: accepted segments decoded, matched to their flow and their
                  payload copied into the flow's contiguous receive window on the device (also
                  ``batch.*``);
* ``flow``      — TCP flow update and ACK build: tcp_input's Established path over the placement's
                  records, per flow in batch order, and the pure ACKs it sends, on the device; the
                  same walk on the host for what the device stops at (also ``batch.*``);
* ``send``      — TCP send planning: tcp_write's window gate and retransmit over the flow records on
                  the device, into the segmentation offload's descriptors; the same plan on the host
                  (also ``batch.*``);
* ``icmp``      — ICMP echo responder: every accepted echo request of a receive batch becomes a finished
                  reply in a transmit pool on the device, buffers drawn from a free list; the same on
                  the host for what the device leaves (also ``batch.*``);
* ``udp``       — UDP receive demux: every accepted UDP datagram to a bound port becomes a record and a
                  payload in its socket's queue on the device, the queues contiguous and in arrival order;
                  the same on the host for what the device leaves — and the UDP send build: every record
                  read as a send becomes a finished datagram in a transmit pool (also ``batch.*``);
* ``listen``    — TCP listen responder: every segment the placement decoded without a flow is answered on the
                  device — RST|ACK for a stray, SYN|ACK and an accept record for a new connection — in batch
                  order; the same on the host for what the device leaves (also ``batch.*``);
* ``workloads`` — the synthetic packet batches BASELINE.json's configs name.
"""
from . import _lib, util  # noqa: F401
from ._lib import ChecksumError, ChecksumLibraryMissing  # noqa: F401

__all__ = ["util", "batch", "pool", "segment", "place", "flow", "send", "icmp", "udp", "listen", "workloads", "ChecksumError",
           "ChecksumLibraryMissing"]


def __getattr__(name):
    if name in ("batch", "pool", "segment", "place", "flow", "send", "icmp", "udp", "listen", "workloads"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
