"""Device time of the widened §8f operations on MI355X (one GPU), next to the plain
batch checksum, on the headline batch (2^20 x 1500 B) and on IMIX:

* csum     — rns_csum_batch_dev (the hot path itself)
* chain    — rns_csum_chain_dev: every packet as the stack receives it after the
             IP trim, three fragments [492, 512, 496]
* fill     — rns_csum_fill_dev: transmit fill of the TCP checksum field [16..18]
* fill_packed — rns_csum_fill_packed_dev: the same fill with the packed descriptors
* verify   — rns_rx_verify_dev: IPv4 header + TCP checks of whole datagrams
* tx       — rns_tx_fill_dev: IPv4 header + TCP checksums of whole datagrams stored in
             place, pseudo-headers formed on the device
* tx_packed — rns_tx_fill_packed_dev: the same finalize over the packed form (the rows transmit
             kernel; round 6)
* verify_packed — rns_rx_verify_packed_dev: receive verify over the packed form
* chain_fill — rns_csum_chain_fill_dev on the transmit shape (workloads.tx_chain_layout:
             20-byte TCP head fragments back to back in a header region, the payload as one
             fragment or as 512-byte NetBuffer fragments), next to the plain chain checksum
             of the same chains (chain_tx)
* tx_chain — rns_tx_fill_chain_dev: whole-datagram finalize of the same transmit shape with
             40-byte IPv4 + TCP head fragments (the layout alloc_header builds, buf.rs:262-291),
             payload as one fragment or 512-byte NetBuffer fragments (round 6)
* tx_chain_packed — rns_tx_fill_chain_packed_dev: the same finalize of the same arena (one payload
             fragment) over the compact descriptors, 3 B per datagram + 16 B per 64 instead of 28 B;
             timed in rounds alternating with tx_chain's, and both rows carry every round's time
* rx_verify_chain — rns_rx_verify_chain_dev: receive verify of the datagrams as recv_packet leaves
             them, NetBuffer chains in 512-byte pool buffers (workloads.RxChainBatch), the buffers in
             order and shuffled; next to it csum_chain, rns_csum_chain_dev over the same chains of the
             same arena (the yardstick: an entry that reads the same bytes), timed in alternating
             rounds, both rows carrying every round's time
* rx_verify_pool — rns_rx_verify_pool_dev: the same receive verify of the same pools over the compact
             descriptors (a u32 buffer index per fragment, a u16 length per datagram, one u32 per 64
             datagrams), next to rns_rx_verify_chain_dev over the CSR chains (the yardstick), in
             alternating rounds; statuses and L4 values are compared before timing
* tx_pool — rns_tx_fill_pool_dev: transmit finalize of datagrams in 512-byte pool buffers as the
             reference's transmit path leaves them (workloads.TxPoolBatch: a 40-byte head at the end of
             its own buffer, the payload in whole buffers and a last partly filled one), the buffers in
             order and shuffled, over the compact descriptors; next to it rns_tx_fill_chain_dev over the
             CSR chains of the same pool tensor (the yardstick), in alternating rounds; bytes and
             statuses are compared before timing
* tx_segment — rns_tx_segment_dev: TCP segmentation offload over workloads.TxSegmentBatch's shapes
             (bulk44: 2^20 segments of mss 1460 as sends of 44 segments, IPv4 40-byte heads; imix1: 2^23
             one-segment sends with IMIX data lengths, the flow search's worst case); next to it
             rns_tx_fill_chain_packed_dev finalizing the same datagrams from prebuilt heads (payloads
             repacked to 16-byte starts), in alternating rounds; both rows carry the descriptor and
             host-to-device bytes per datagram.  Timed once per run, whatever --configs names
* rx_place — rns_rx_tcp_place_pool_dev: TCP receive placement over RxPlaceBatch's shapes (bulk: 2^20
             datagrams of 1500 B, 1024 flows x 1024 in-order segments of 1460 B; imix: 2^23 IMIX datagrams
             whose 40-byte ones are pure ACKs, decoded and not placed), in 512-byte buffers in order and
             shuffled; next to it rns_rx_verify_pool_dev on the same pool (the difference is what decode,
             lookup and copy cost) and that verify plus a plain device-to-device copy of the payload bytes
             (the floor of a two-pass design on payloads that were already contiguous), in alternating
             rounds; every row carries descriptor bytes and read / written bytes per datagram.  Timed once
             per run, whatever --configs names
* rx_flow  — rns_rx_tcp_flow_update_dev + rns_tx_ack_build_dev behind the placement, over RxPlaceBatch's
             shapes in order (the records do not depend on the buffers' order), the flows' state set so
             that every segment is consumed; a flow takes at most RNS_FLOW_MAX_SEGS segments per call, so
             a batch with more per flow (imix: 8192) goes through in slices of flows x 1024 datagrams
             with the state carried.  Timed in alternating rounds: the placement alone, the update
             alone, the build alone and all three; and, for the other extreme, 2^20 flows with one
             synthetic segment each.  The rows carry the added passes as a ratio to the placement and
             their record traffic against the floor of 24 B read + 8 B written per datagram
* tx_plan  — rns_tx_tcp_plan_dev in front of rns_tx_segment_dev: flows with nothing in flight, an open
             window and k whole segments of 1460 bytes queued (1024 flows x 44, and 2^20 flows x 1), no
             retransmits.  Timed in alternating rounds: (a) the segmentation alone from descriptors over
             the flows that the host laid out beforehand (rns_tx_segment_layout, templates patched on the
             host), (b) the plan and then the segmentation on the planned descriptors, (c) the plan
             alone; the head bytes of (a) and (b) are compared before timing.  Timed once per run,
             whatever --configs names
* rx_echo  — rns_rx_icmp_echo_pool_dev: 2^20 IPv4 pings of 84 bytes, 2^20 of 1500 bytes, and 2^23
             IMIX-sized datagrams (40 / 576 / 1500 at 7:4:1) of which every fourth is a ping and the rest
             UDP, in 512-byte buffers.  Timed in alternating rounds: (a) the responder, (b) the pool verify
             alone, (c) the pool verify and then rns_tx_fill_pool_dev over prebuilt replies of the same
             shapes — the floor that copies nothing; the replies of (a) are compared with echo_host on a
             sample before timing.  Timed once per run, whatever --configs names
* rx_udp   — rns_rx_udp_demux_pool_dev: 2^20 UDP datagrams of 1500 bytes over 1024 sockets, 2^20 of 64 bytes
             to one socket, and 2^23 IMIX-sized ones (workloads.imix_lengths) over 16 sockets, IPv4 in 512-byte
             buffers, the sockets interleaved.  Timed in alternating rounds: (a) the demux, (b) the pool verify
             alone, (c) rns_rx_tcp_place_pool_dev over RxPlaceBatch's TCP segments of the same datagram sizes
             (1500: 1460 payload bytes against the demux's 1472; none for the 64-byte shape) — the nearest
             existing copy; the queues of (a) are checked on the device before timing: d_q_first against the
             sockets' counts, and every record and payload of a sample.  Timed once per run, whatever
             --configs names
* tx_udp   — rns_tx_udp_send_pool_dev over the demux's own records and payloads (an echo server's sends):
             2^20 sends of 1472 bytes from 1024 sockets, 2^20 of 64 bytes from one socket, and 2^23 IMIX-sized
             ones (workloads.imix_lengths less 28 header bytes) from 16 sockets, IPv4 into 512-byte buffers
             drawn from a shuffled free list.  Timed in alternating rounds: (a) the send build, (b)
             rns_tx_fill_pool_dev over the datagrams it built — the floor that copies nothing, (c) the demux
             and then the send build, (d) the demux alone, (e) a plain device copy of the payload bytes; the
             datagrams of (a) are compared with send_host on a sample before timing.  Timed once per run,
             whatever --configs names
* rx_listen — rns_rx_tcp_listen_pool_dev behind the placement: 2^20 IPv4 SYNs with an MSS option from distinct sources
             to one listening port, 2^20 stray 40-byte segments (all RSTs), and 2^23 IMIX-sized datagrams over 1024
             known flows with 1 % SYNs and 1 % strays, in 512-byte buffers.  Timed in alternating rounds: (a) the
             responder, (b) verify + placement alone (the launches it follows), (c) both, (d) rns_tx_ack_build_dev
             over the same number of heads — the floor that classifies nothing; counts, d_conn and the replies and
             accept records of the first 4096 datagrams are compared with listen_host before timing.  Timed once per
             run, whatever --configs names
* rx_conn  — rns_rx_tcp_conn_update_dev against rns_rx_tcp_flow_update_dev, and the close lifecycle: (a) rx_flow's
             own bulk shape (behind the placement) and its 2^20-flows shape through both updates in alternating
             rounds: the cost of the wider step on traffic that needs none of it; (b) 2^20 SynReceived flows, one
             handshake-completing ACK each (the lane path); (c) 2^18 flows x 4 segments — ACK, request, FIN|ACK,
             and after rns_tx_tcp_close_dev the last ACK in a second call — followed by rns_tx_tcp_ctl_build_dev.
             The records, flows and results of a sample are compared with conn_update_host before timing.  Timed
             once per run, whatever --configs names

Timing: one pair of HIP events around K back-to-back launches on the launch stream,
median of R rounds.  GB/s counts algorithmic bytes (payload read + result bytes
written); descriptor and workspace traffic is not credited.

    python tools/bench_ops.py [--steps 20] [--rounds 5] [--out profiles/archive/r01/r01_ops.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rustnetworkstack_amd.batch import (PreparedBatch, csum_chain, csum_fill, csum_fill_packed,  # noqa: E402
                                        packed_layout, rx_verify, rx_verify_packed, tx_fill, tx_fill_packed)
from rustnetworkstack_amd.workloads import DeviceBatch, make_layout  # noqa: E402

L4 = bytes([192, 168, 1, 2])
L6 = bytes.fromhex("fe800000000000000000000000000002")


def write_ipv4_tcp_headers(b, lay, dev):
    """IPv4 header (src R4, dst L4, proto 6) in each packet's first 20 bytes, header
    checksum filled (ip.rs:158-159), TCP checksum filled with the per-packet
    pseudo-header seed (tcp.rs:957-973)."""
    from oracle.oracle import pseudo_header_py  # test infrastructure: builds inputs only
    n = lay.n
    hdr = np.frombuffer(bytes.fromhex("4500000000004000400600000000000000000000"), dtype=np.uint8).copy()
    hdr[12:16] = [192, 168, 1, 1]
    hdr[16:20] = np.frombuffer(L4, dtype=np.uint8)
    hdrs = np.tile(hdr, (n, 1))
    hdrs[:, 2] = (lay.length >> 8) & 0xFF
    hdrs[:, 3] = lay.length & 0xFF
    idx = b.off.view(-1, 1) + torch.arange(20, device=dev)
    b.arena[idx.flatten()] = torch.from_numpy(hdrs.reshape(-1)).to(dev)
    del idx
    csum_fill(b.arena, b.off, torch.full((n,), 20, dtype=torch.int32, device=dev), None, field_off=10)
    l4 = lay.length.astype(np.int64) - 20
    uniq = {int(x): pseudo_header_py(bytes([192, 168, 1, 1]), L4, int(x), 6) for x in np.unique(l4)}
    seeds = np.array([uniq[int(x)] for x in l4], dtype=np.uint16) if len(uniq) > 1 else \
        np.full(n, next(iter(uniq.values())), dtype=np.uint16)
    csum_fill(b.arena, b.off + 20, b.length - 20, torch.from_numpy(seeds.view(np.int16)).to(dev), field_off=16)
    torch.cuda.synchronize()


def timed_rounds(fns, steps, rounds):
    """Every round's ms per launch (sorted) of each function; the rounds of several functions
    alternate, so they see the same machine."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns:
        fn()
        fn()
    res = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / steps)
    return [sorted(r) for r in res]


def timed(fn, steps, rounds):
    res = timed_rounds([fn], steps, rounds)[0]
    return res[len(res) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="c3_1500B,c5_imix")
    ap.add_argument("--ops", default="csum,chain,fill,verify,tx")
    ap.add_argument("--out", default="")
    ap.add_argument("--chain-layouts", default="packed,netbuf,netbuf_shuffled",
                    help="packed: [492, 512, rest] fragments back to back inside each packet; netbuf: every "
                         "fragment in its own 512-byte buffer (NetBuffer, buf.rs:50), ceil(L/512) per packet, "
                         "the buffers in order (a packet's fragments adjacent); netbuf_shuffled: the same "
                         "buffers in a random order (no two fragments adjacent)")
    ap.add_argument("--tx-frags", default="0,512", help="chain_fill: payload fragment sizes (0 = one fragment)")
    ap.add_argument("--segment-shapes", default="bulk44,imix1", help="tx_segment: workloads.TxSegmentBatch shapes")
    ap.add_argument("--segment-n", type=int, default=0, help="tx_segment: segments per shape (0 = the shape's default)")
    ap.add_argument("--place-shapes", default="bulk,imix", help="rx_place: bulk (1500-byte datagrams) and / or imix")
    ap.add_argument("--place-n", type=int, default=0, help="rx_place: datagrams per shape (0 = 2^20 bulk, 2^23 imix)")
    ap.add_argument("--place-flows", type=int, default=1024, help="rx_place: flows (a divisor of the datagram count)")
    ap.add_argument("--echo-shapes", default="ping84,ping1500,imix", help="rx_echo: the shapes to time")
    ap.add_argument("--echo-n", type=int, default=0, help="rx_echo: datagrams per shape (0 = 2^20 pings, 2^23 imix)")
    ap.add_argument("--udp-shapes", default="udp1500:1024,udp64:1,imix:16", help="rx_udp: shape:sockets to time")
    ap.add_argument("--udp-n", type=int, default=0, help="rx_udp, tx_udp: datagrams per shape (0 = 2^20, 2^23 imix)")
    ap.add_argument("--tx-udp-shapes", default="udp1472:1024,udp64:1,imix:16", help="tx_udp: shape (payload bytes):sockets to time")
    ap.add_argument("--listen-shapes", default="syn,stray,imix", help="rx_listen: the shapes to time")
    ap.add_argument("--listen-n", type=int, default=0, help="rx_listen: datagrams per shape (0 = 2^20 syn / stray, 2^23 imix)")
    ap.add_argument("--tx-modes", default="plain,runs,txpacked", help="chain_fill: hint flags to time")
    args = ap.parse_args()
    ops = set(args.ops.split(","))
    dev = torch.device("cuda:0")
    results = {}
    for cfg in args.configs.split(","):
        lay = make_layout(cfg)
        b = DeviceBatch(lay, dev)
        n, pay = lay.n, lay.payload_bytes
        r = {}
        pb = PreparedBatch(b.arena, b.off, b.length, b.seed, complement=True, out=b.out,
                           len_hint=int(round(lay.mean_len)))
        if "csum" in ops:
            ms = timed(pb, args.steps, args.rounds)
            r["csum"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1)}
        if "chain" in ops:
            for cl in args.chain_layouts.split(","):
                key = "chain" if cl == "packed" else f"chain_{cl}"
                for runs in (False, True):  # without / with RNS_FLAG_CHAIN_RUNS
                    r[key + ("_runs" if runs else "")] = bench_chain(b, lay, dev, args, runs) if cl == "packed" else \
                        bench_chain_netbuf(lay, dev, args, shuffled=cl == "netbuf_shuffled", runs=runs)
        if "chain_fill" in ops:
            for frag in (int(x) for x in args.tx_frags.split(",")):
                r.update(bench_chain_fill(cfg, dev, args, frag))
        if "tx_chain" in ops or "tx_chain_packed" in ops:
            for frag in (int(x) for x in args.tx_frags.split(",")):
                if "tx_chain" in ops or frag == 0:
                    r.update(bench_tx_chain(cfg, dev, args, frag, packed="tx_chain_packed" in ops and frag == 0))
        if "rx_verify_chain" in ops:
            for shuffled in (False, True):
                r.update(bench_rx_chain(cfg, dev, args, shuffled))
        if "rx_verify_pool" in ops:
            for shuffled in (False, True):
                r.update(bench_rx_pool(cfg, dev, args, shuffled))
        if "tx_pool" in ops:
            for shuffled in (False, True):
                r.update(bench_tx_pool(cfg, dev, args, shuffled))
        if "tx_segment" in ops and cfg == args.configs.split(",")[0]:  # its shapes are its own, not the configs'
            for shape in args.segment_shapes.split(","):
                r.update(bench_tx_segment(shape, dev, args))
        if "rx_place" in ops and cfg == args.configs.split(",")[0]:  # its shapes are its own, too
            for shape in args.place_shapes.split(","):
                for shuffled in (False, True):
                    r.update(bench_rx_place(shape, dev, args, shuffled))
        if "rx_flow" in ops and cfg == args.configs.split(",")[0]:
            for shape in args.place_shapes.split(","):
                r.update(bench_rx_flow(shape, dev, args))
            r.update(bench_rx_flow_wide(dev, args))
        if "rx_conn" in ops and cfg == args.configs.split(",")[0]:
            r.update(bench_rx_conn_bulk(dev, args))
            r.update(bench_rx_conn_wide(dev, args))
            r.update(bench_rx_conn_handshake(dev, args))
            r.update(bench_rx_conn_lifecycle(dev, args))
        if "tx_plan" in ops and cfg == args.configs.split(",")[0]:
            for nfl, k in ((1024, 44), (1 << 20, 1)):
                r.update(bench_tx_plan(nfl, k, dev, args))
        if "rx_echo" in ops and cfg == args.configs.split(",")[0]:
            for shape in args.echo_shapes.split(","):
                r.update(bench_rx_echo(shape, dev, args))
        if "rx_udp" in ops and cfg == args.configs.split(",")[0]:
            for spec in args.udp_shapes.split(","):
                shape, socks = spec.split(":")
                r.update(bench_rx_udp(shape, int(socks), dev, args))
        if "tx_udp" in ops and cfg == args.configs.split(",")[0]:
            for spec in args.tx_udp_shapes.split(","):
                shape, socks = spec.split(":")
                r.update(bench_tx_udp(shape, int(socks), dev, args))
        if "rx_listen" in ops and cfg == args.configs.split(",")[0]:
            for shape in args.listen_shapes.split(","):
                r.update(bench_rx_listen(shape, dev, args))
        if "fill" in ops:
            ms = timed(lambda: csum_fill(b.arena, b.off, b.length, b.seed, field_off=16), args.steps, args.rounds)
            r["fill"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1)}
        if "fill_packed" in ops:
            blk, _, _ = packed_layout(lay.length, align_log2=4)
            blk_t = torch.from_numpy(blk.view(np.int64)).to(dev)
            len16 = torch.from_numpy(lay.length.astype(np.uint16).view(np.int16)).to(dev)
            hint = int(round(lay.mean_len))
            ms = timed(lambda: csum_fill_packed(b.arena, blk_t, len16, b.seed, align_log2=4, field_off=16,
                                                len_hint=hint), args.steps, args.rounds)
            r["fill_packed"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1)}
        if "tx" in ops:
            write_ipv4_tcp_headers(b, lay, dev)
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            ms = timed(lambda: tx_fill(b.arena, b.off, b.length, status=st), args.steps, args.rounds)
            filled = int((st == 3).sum().item())
            r["tx"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + n) / ms / 1e6, 1), "filled": filled,
                       "packets": n}
        if "tx_packed" in ops:
            write_ipv4_tcp_headers(b, lay, dev)
            b.launcher(packed=True)  # uploads blk_off / len16
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            hint = int(round(lay.mean_len))
            ms = timed(lambda: tx_fill_packed(b.arena, b.blk_off, b.len16, status=st, len_hint=hint),
                       args.steps, args.rounds)
            filled = int((st == 3).sum().item())
            r["tx_packed"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + n) / ms / 1e6, 1), "filled": filled,
                              "packets": n}
        if "verify_packed" in ops:
            write_ipv4_tcp_headers(b, lay, dev)
            b.launcher(packed=True)
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            ms = timed(lambda: rx_verify_packed(b.arena, b.blk_off, b.len16, L4, L6, status=st),
                       args.steps, args.rounds)
            accepted = int((st == 0x43).sum().item())
            r["verify_packed"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + n) / ms / 1e6, 1),
                                  "accepted": accepted, "packets": n}
        if "verify" in ops:
            # turn every packet into a valid IPv4/TCP datagram first (header written
            # on the GPU, IPv4 and TCP checksums filled), so every byte is checked
            write_ipv4_tcp_headers(b, lay, dev)
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            ms = timed(lambda: rx_verify(b.arena, b.off, b.length, L4, L6, status=st),
                       args.steps, args.rounds)
            accepted = int((st == 0x43).sum().item())
            r["verify"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + n) / ms / 1e6, 1),
                           "accepted": accepted, "packets": n}
        results[cfg] = r
        print(cfg, json.dumps(r), flush=True)
        del b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_ops.py", "steps": args.steps, "rounds": args.rounds,
                       "results": results}, f, indent=1)
    print(json.dumps(results))


def bench_chain(b, lay, dev, args, runs=False):
    n, pay = lay.n, lay.payload_bytes
    # chain: three fragments per packet where the packet is long enough, else one
    L = lay.length.astype(np.int64)
    nfr = np.where(L > 1004, 3, 1)
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nfr, out=first[1:])
    nf = int(first[-1])
    frag_off = np.empty(nf, dtype=np.uint64)
    frag_len = np.empty(nf, dtype=np.uint32)
    three = nfr == 3
    i3 = first[:-1][three]
    frag_off[i3] = lay.off[three]
    frag_off[i3 + 1] = lay.off[three] + 492
    frag_off[i3 + 2] = lay.off[three] + 1004
    frag_len[i3] = 492
    frag_len[i3 + 1] = 512
    frag_len[i3 + 2] = (L[three] - 1004).astype(np.uint32)
    i1 = first[:-1][~three]
    frag_off[i1] = lay.off[~three]
    frag_len[i1] = lay.length[~three]
    d_fo = torch.from_numpy(frag_off.view(np.int64)).to(dev)
    d_fl = torch.from_numpy(frag_len.view(np.int32)).to(dev)
    d_first = torch.from_numpy(first.astype(np.uint32).view(np.int32)).to(dev)
    sums = torch.empty(nf, dtype=torch.uint16, device=dev)
    out = torch.empty(n, dtype=torch.uint16, device=dev)
    ms = timed(lambda: csum_chain(b.arena, d_fo, d_fl, d_first, b.seed, complement=True, out=out,
                                  frag_sums=sums, frag_len_hint=int(round(pay / nf)), runs=runs),
               args.steps, args.rounds)
    return {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1), "fragments": nf}


def bench_chain_fill(cfg, dev, args, frag):
    """The head-fragment fill and the plain chain checksum over the transmit shape."""
    from rustnetworkstack_amd.batch import csum_chain_fill, fill_splitmix64
    from rustnetworkstack_amd.workloads import tx_chain_layout
    t = tx_chain_layout(cfg, frag=frag)
    n, pay, nf = t.n, t.payload_bytes, int(t.frag_off.shape[0])
    arena = torch.empty(t.arena_bytes + 64, dtype=torch.uint8, device=dev)
    fill_splitmix64(arena, t.data_seed)
    d_fo = torch.from_numpy(t.frag_off.view(np.int64)).to(dev)
    d_fl = torch.from_numpy(t.frag_len.view(np.int32)).to(dev)
    d_first = torch.from_numpy(t.first.view(np.int32)).to(dev)
    seed = torch.from_numpy(t.seed.view(np.int16)).to(dev)
    out = torch.empty(n, dtype=torch.uint16, device=dev)
    hint = int(round(pay / nf))
    tag = "tx" if frag == 0 else f"tx{frag}"
    res = {}
    modes = {"plain": (False, False), "runs": (True, False), "txpacked": (False, True)}
    for runs, txp in (modes[m] for m in args.tx_modes.split(",")):
        sfx = "_runs" if runs else "_txpacked" if txp else ""
        ms = timed(lambda: csum_chain_fill(arena, d_fo, d_fl, d_first, seed, field_off=t.field, out=out,
                                           frag_len_hint=hint, runs=runs, tx_packed=txp), args.steps, args.rounds)
        res[f"chain_fill_{tag}{sfx}"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1),
                                        "fragments": nf, "hint": hint}
        ms = timed(lambda: csum_chain(arena, d_fo, d_fl, d_first, seed, complement=True, out=out,
                                      frag_len_hint=hint, runs=runs, tx_packed=txp), args.steps, args.rounds)
        res[f"chain_{tag}{sfx}"] = {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1)}
    del arena
    torch.cuda.empty_cache()
    return res


def bench_tx_chain(cfg, dev, args, frag, packed=False):
    """Whole-datagram transmit finalize over NetBuffer chains: 40-byte IPv4 + TCP heads back to
    back in a header region, payloads packed at 16-byte starts (one fragment, or 512-byte ones).
    packed: also the compact-descriptor entry over the same arena, its rounds alternating with the
    CSR entry's (the finalize is idempotent: both store the same bytes every launch)."""
    from rustnetworkstack_amd.batch import fill_splitmix64, tx_fill_chain, tx_fill_chain_packed
    from rustnetworkstack_amd.workloads import tx_chain_compact, tx_chain_layout
    t = tx_chain_layout(cfg, head=40, frag=frag)
    n, pay, nf = t.n, t.payload_bytes, int(t.frag_off.shape[0])
    arena = torch.empty(t.arena_bytes + 64, dtype=torch.uint8, device=dev)
    fill_splitmix64(arena, t.data_seed)
    hoff = torch.from_numpy(t.frag_off[t.first[:-1].astype(np.int64)].view(np.int64)).to(dev)
    hdr = np.frombuffer(bytes.fromhex("4500000000004000400600000000000000000000"), dtype=np.uint8).copy()
    hdr[12:16] = [192, 168, 1, 1]
    hdr[16:20] = np.frombuffer(L4, dtype=np.uint8)
    idx = hoff.view(-1, 1) + torch.arange(20, device=dev)
    arena[idx.flatten()] = torch.from_numpy(hdr).to(dev).repeat(n)
    del idx
    d_fo = torch.from_numpy(t.frag_off.view(np.int64)).to(dev)
    d_fl = torch.from_numpy(t.frag_len.view(np.int32)).to(dev)
    d_first = torch.from_numpy(t.first.view(np.int32)).to(dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    tag = "tx_chain" if frag == 0 else f"tx_chain{frag}"

    def row(rs, desc_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "GBps": round((pay + n) / ms / 1e6, 1), "filled": int((st == 3).sum().item()),
                "packets": n, "fragments": nf, "rounds_us": [round(x * 1e3, 1) for x in rs],
                "spread_us": round((rs[-1] - rs[0]) * 1e3, 1), "descriptor_bytes": desc_bytes}

    csr = lambda: tx_fill_chain(arena, d_fo, d_fl, d_first, status=st)  # noqa: E731
    res = {}
    if packed:
        hblk, hl8, pblk, pl16 = tx_chain_compact(t)
        d_hblk, d_hl8 = torch.from_numpy(hblk.view(np.int64)).to(dev), torch.from_numpy(hl8).to(dev)
        d_pblk, d_pl16 = torch.from_numpy(pblk.view(np.int64)).to(dev), torch.from_numpy(pl16.view(np.int16)).to(dev)
        st2 = torch.empty_like(st)
        cpt = lambda: tx_fill_chain_packed(arena, d_hblk, d_hl8, d_pblk, d_pl16, status=st2)  # noqa: E731
        # both entries from the same unfinalized header region: the bytes stored must be identical
        hreg = int(pblk[0])  # the header region ends below the first payload
        before = arena[:hreg].clone()
        csr()
        heads_csr = arena[:hreg].clone()
        arena[:hreg].copy_(before)
        cpt()
        same = bool(torch.equal(arena[:hreg], heads_csr)) and bool(torch.equal(st, st2))
        del before, heads_csr
        rs_csr, rs_cpt = timed_rounds([csr, cpt], args.steps, args.rounds)
        res[tag] = row(rs_csr, 12 * nf + 4 * (n + 1))
        res["tx_chain_packed"] = row(rs_cpt, 3 * n + 16 * ((n + 63) // 64))
        res["tx_chain_packed"]["bytes_and_status_equal_csr"] = same
        med_csr, med_cpt = rs_csr[len(rs_csr) // 2], rs_cpt[len(rs_cpt) // 2]
        res["tx_chain_packed"]["within_csr_median_plus_spread"] = bool(med_cpt <= med_csr + (rs_csr[-1] - rs_csr[0]))
    else:
        res[tag] = row(timed_rounds([csr], args.steps, args.rounds)[0], 12 * nf + 4 * (n + 1))
    del arena
    torch.cuda.empty_cache()
    return res


def bench_rx_chain(cfg, dev, args, shuffled):
    """Receive verify over NetBuffer chains and the plain chain checksum of the same chains, in
    alternating rounds on one arena."""
    from rustnetworkstack_amd.batch import rx_verify_chain
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6, RxChainBatch
    rb = RxChainBatch(cfg, dev, shuffled=shuffled)
    n, pay, nf = rb.n, rb.payload_bytes, rb.n_frags
    out = torch.empty(n, dtype=torch.uint16, device=dev)
    hint = int(round(pay / nf))
    rx = lambda: rx_verify_chain(rb.arena, rb.d_off, rb.d_len, rb.d_first, LOCAL4, LOCAL6,  # noqa: E731
                                 status=rb.status, l4_sum=rb.l4_sum)
    cs = lambda: csum_chain(rb.arena, rb.d_off, rb.d_len, rb.d_first, None, complement=True, out=out,  # noqa: E731
                            frag_len_hint=hint)
    rx()
    torch.cuda.synchronize()
    st = rb.status.cpu().numpy()
    as_expected = bool(np.array_equal(st, rb.expected_status))
    rs_rx, rs_cs = timed_rounds([rx, cs], args.steps, args.rounds)

    def row(rs, result_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "GBps": round((pay + result_bytes) / ms / 1e6, 1), "packets": n,
                "fragments": nf, "rounds_us": [round(x * 1e3, 1) for x in rs],
                "spread_us": round((rs[-1] - rs[0]) * 1e3, 1)}

    tag = "_shuffled" if shuffled else ""
    res = {"rx_verify_chain" + tag: row(rs_rx, 3 * n), "csum_chain" + tag: row(rs_cs, 2 * n)}
    rxr = res["rx_verify_chain" + tag]
    rxr["accepted"] = int((st == 0x43).sum())
    rxr["statuses_as_expected"] = as_expected
    rxr["ratio_to_csum_chain"] = round(rs_rx[len(rs_rx) // 2] / rs_cs[len(rs_cs) // 2], 4)
    del rb
    torch.cuda.empty_cache()
    return res


def bench_rx_pool(cfg, dev, args, shuffled):
    """Receive verify over the compact pool descriptors and over the CSR chains of the same pool, in
    alternating rounds."""
    from rustnetworkstack_amd.batch import rx_verify_chain, rx_verify_pool
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6, RxChainBatch
    rb = RxChainBatch(cfg, dev, shuffled=shuffled)
    n, pay, nf = rb.n, rb.payload_bytes, rb.n_frags
    st_c, l4_c = torch.empty_like(rb.status), torch.empty_like(rb.l4_sum)
    pool = lambda: rx_verify_pool(rb.arena, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6,  # noqa: E731
                                  buf_bytes=rb.layout.buf_bytes, status=rb.status, l4_sum=rb.l4_sum)
    chain = lambda: rx_verify_chain(rb.arena, rb.d_off, rb.d_len, rb.d_first, LOCAL4, LOCAL6,  # noqa: E731
                                    status=st_c, l4_sum=l4_c)
    pool()
    chain()
    torch.cuda.synchronize()
    st = rb.status.cpu().numpy()
    as_expected = bool(np.array_equal(st, rb.expected_status))
    equal = bool(torch.equal(rb.status, st_c)) and bool(torch.equal(rb.l4_sum.view(torch.int16), l4_c.view(torch.int16)))
    rs_p, rs_c = timed_rounds([pool, chain], args.steps, args.rounds)

    def row(rs, desc_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "GBps": round((pay + 3 * n) / ms / 1e6, 1), "packets": n, "fragments": nf,
                "rounds_us": [round(x * 1e3, 1) for x in rs], "spread_us": round((rs[-1] - rs[0]) * 1e3, 1),
                "descriptor_bytes_per_datagram": round(desc_bytes / n, 2)}

    tag = "_shuffled" if shuffled else ""
    res = {"rx_verify_pool" + tag: row(rs_p, 4 * nf + 2 * n + 4 * ((n + 63) // 64)),
           "rx_verify_chain" + tag: row(rs_c, 12 * nf + 4 * (n + 1))}
    pr = res["rx_verify_pool" + tag]
    pr["accepted"] = int((st == 0x43).sum())
    pr["statuses_as_expected"] = as_expected
    pr["status_and_l4_equal_chain"] = equal
    med_p, med_c = rs_p[len(rs_p) // 2], rs_c[len(rs_c) // 2]
    pr["ratio_to_rx_verify_chain"] = round(med_p / med_c, 4)
    pr["within_chain_median_plus_spread"] = bool(med_p <= med_c + max(rs_c[-1] - rs_c[0], rs_p[-1] - rs_p[0]))
    del rb
    torch.cuda.empty_cache()
    return res


def bench_tx_pool(cfg, dev, args, shuffled):
    """Transmit finalize over the compact pool descriptors and over the CSR chains of the same pool, in
    alternating rounds (finalizing again stores the same bytes, so both run on one tensor)."""
    from rustnetworkstack_amd.batch import tx_fill_chain, tx_fill_pool
    from rustnetworkstack_amd.workloads import TxPoolBatch
    tb = TxPoolBatch(cfg, dev, shuffled=shuffled)
    n, pay, nf = tb.n, tb.payload_bytes, tb.n_frags
    st_c = torch.empty_like(tb.status)
    pool = lambda: tx_fill_pool(tb.arena, tb.d_buf_idx, tb.d_blk_first, tb.d_head_len8, tb.d_pay_len16,  # noqa: E731
                                buf_bytes=tb.buf_bytes, status=tb.status)
    chain = lambda: tx_fill_chain(tb.arena, tb.d_off, tb.d_len, tb.d_first, status=st_c)  # noqa: E731
    # the two entries' bytes, each from the unfinalized pool (the heads are all either writes)
    heads = torch.from_numpy(tb.hoff).to(dev).view(-1, 1) + torch.arange(tb.HEAD, device=dev)
    raw = tb.arena[heads.flatten()].clone()
    pool()
    torch.cuda.synchronize()
    by_pool = tb.arena[heads.flatten()].clone()
    tb.arena[heads.flatten()] = raw
    chain()
    torch.cuda.synchronize()
    equal = bool(torch.equal(tb.arena[heads.flatten()], by_pool)) and bool(torch.equal(tb.status, st_c))
    changed = not bool(torch.equal(by_pool, raw))
    del heads, raw, by_pool
    filled = int((tb.status == 3).sum().item())
    rs_p, rs_c = timed_rounds([pool, chain], args.steps, args.rounds)

    def row(rs, desc_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "GBps": round((pay + 5 * n) / ms / 1e6, 1), "packets": n, "fragments": nf,
                "rounds_us": [round(x * 1e3, 1) for x in rs], "spread_us": round((rs[-1] - rs[0]) * 1e3, 1),
                "descriptor_bytes_per_datagram": round(desc_bytes / n, 2)}

    tag = "_shuffled" if shuffled else ""
    res = {"tx_pool" + tag: row(rs_p, 3 * n + 4 * nf + 4 * ((n + 63) // 64)),
           "tx_pool_chain" + tag: row(rs_c, 12 * nf + 4 * (n + 1))}
    pr = res["tx_pool" + tag]
    pr["filled"] = filled
    pr["heads_changed"] = changed
    pr["bytes_and_status_equal_chain"] = equal
    med_p, med_c = rs_p[len(rs_p) // 2], rs_c[len(rs_c) // 2]
    spread = max(rs_c[-1] - rs_c[0], rs_p[-1] - rs_p[0])
    pr["ratio_to_tx_fill_chain"] = round(med_p / med_c, 4)
    pr["faster_than_chain_by_more_than_spread"] = bool(med_p < med_c - spread)
    pr["within_chain_median_plus_spread"] = bool(med_p <= med_c + spread)
    del tb
    torch.cuda.empty_cache()
    return res


def bench_tx_segment(shape, dev, args):
    """TCP segmentation offload against the compact chain finalize of the same datagrams from prebuilt
    heads (the best path without it), in alternating rounds; both rewrite the same bytes every time."""
    from rustnetworkstack_amd.batch import tx_fill_chain_packed, tx_segment
    from rustnetworkstack_amd.workloads import TxSegmentBatch
    tb = TxSegmentBatch(shape, dev, n_seg=args.segment_n or None)
    n, pay = tb.n, tb.payload_bytes
    seg = lambda: tx_segment(tb.arena, tb.d_tmpl, tb.d_head_len8, tb.d_pay_off, tb.d_pay_len, tb.d_mss,  # noqa: E731
                             tb.d_head_off, tb.d_seg_first, tb.d_blk_flow, n, status=tb.status)
    cpt = lambda: tx_fill_chain_packed(tb.c_arena, tb.c_head_blk_off, tb.c_head_len8, tb.c_pay_blk_off,  # noqa: E731
                                       tb.c_pay_len16, pay_align_log2=4, status=tb.c_status)
    seg()
    cpt()
    torch.cuda.synchronize()
    filled, c_filled = int((tb.status == 3).sum().item()), int((tb.c_status == 3).sum().item())
    rs_s, rs_c = timed_rounds([seg, cpt], args.steps, args.rounds)

    def row(rs, desc_bytes, h2d_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "GBps": round(pay / ms / 1e6, 1), "datagrams": n, "flows": tb.n_flows,
                "rounds_us": [round(x * 1e3, 1) for x in rs], "spread_us": round((rs[-1] - rs[0]) * 1e3, 1),
                "descriptor_bytes_per_datagram": round(desc_bytes / n, 3),
                "h2d_bytes_per_datagram": round(h2d_bytes / n, 1)}

    res = {f"tx_segment_{shape}": row(rs_s, tb.desc_bytes, tb.h2d_bytes),
           f"tx_segment_{shape}_compact_finalize": row(rs_c, tb.c_desc_bytes, tb.c_h2d_bytes)}
    pr = res[f"tx_segment_{shape}"]
    pr["filled"], res[f"tx_segment_{shape}_compact_finalize"]["filled"] = filled, c_filled
    med_s, med_c = rs_s[len(rs_s) // 2], rs_c[len(rs_c) // 2]
    spread = max(rs_c[-1] - rs_c[0], rs_s[-1] - rs_s[0])
    pr["ratio_to_compact_finalize"] = round(med_s / med_c, 4)
    pr["within_compact_median_plus_spread"] = bool(med_s <= med_c + spread)
    del tb
    torch.cuda.empty_cache()
    return res


class RxPlaceBatch:
    """Received TCP segments of `n_flows` flows in 512-byte pool buffers, for rns_rx_tcp_place_pool_dev:
    datagram i belongs to flow i % n_flows and carries that flow's next in-order payload bytes.  bulk:
    every datagram 1500 B (1460 B of payload); imix: workloads.imix_lengths, whose 40-byte datagrams are
    pure ACKs.  IPv4, 20-byte headers; the checksums are filled by rns_tx_fill_dev."""

    BUF, HEAD = 512, 40

    def __init__(self, shape, dev, n, n_flows, shuffled):
        from rustnetworkstack_amd.batch import fill_splitmix64, rx_flow_table
        from rustnetworkstack_amd.workloads import DATA_SEED, LOCAL4, SHUFFLE_STREAM, imix_lengths, splitmix64
        B, H = self.BUF, self.HEAD
        assert n % n_flows == 0 and n_flows <= 65536
        length = np.full(n, 1500, dtype=np.int64) if shape == "bulk" else imix_lengths(n, DATA_SEED).astype(np.int64)
        pay = length - H
        nfr = (length + B - 1) // B
        first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(nfr, out=first[1:])
        nf = int(first[-1])
        flow = np.arange(n) % n_flows
        per_flow = pay.reshape(-1, n_flows)                       # row j: the flows' j-th segments
        before = np.cumsum(per_flow, axis=0) - per_flow           # payload bytes of the flow before each
        win_len = per_flow.sum(axis=0)
        win_off = np.concatenate([[0], np.cumsum(win_len)[:-1]])
        next_seq = (0xFFFF0000 + 977 * np.arange(n_flows)) & 0xFFFFFFFF
        seq = (next_seq[flow] + before.reshape(-1)) & 0xFFFFFFFF
        h = np.zeros((n, H), dtype=np.uint8)
        h[:, 0], h[:, 6], h[:, 8], h[:, 9] = 0x45, 0x40, 64, 6
        h[:, 2], h[:, 3] = (length >> 8) & 0xFF, length & 0xFF
        h[:, 12], h[:, 13], h[:, 14], h[:, 15] = 10, 1, flow >> 8, flow & 0xFF
        h[:, 16:20] = np.frombuffer(LOCAL4, dtype=np.uint8)
        sport = 40000 + (flow % 20000)
        h[:, 20], h[:, 21], h[:, 22], h[:, 23] = sport >> 8, sport & 0xFF, 0, 80
        for k in range(4):
            h[:, 24 + k] = (seq >> (24 - 8 * k)) & 0xFF
        h[:, 32], h[:, 33], h[:, 34] = 0x50, 0x18, 0x20                # data offset 5, ACK | PSH, window 0x2000
        self.n, self.n_flows, self.n_frags, self.pay_total = n, n_flows, nf, int(pay.sum())
        self.total_bytes = int(length.sum())
        arena = torch.empty(nf * B + 16, dtype=torch.uint8, device=dev)
        fill_splitmix64(arena[:nf * B], DATA_SEED)
        d_off = torch.from_numpy(first[:-1] * B).to(dev)
        d_h = torch.from_numpy(h).to(dev)
        step = 1 << 20
        for i in range(0, n, step):
            idx = d_off[i:i + step].view(-1, 1) + torch.arange(H, device=dev)
            arena[idx.flatten()] = d_h[i:i + step].flatten()
        del d_h
        st = tx_fill(arena, d_off, torch.from_numpy(length.astype(np.int32)).to(dev))
        assert int((st != 3).sum().item()) == 0, "transmit finalize did not fill every synthetic datagram"
        self.flat, self.flat_off, self.pay, self.flow = arena, first[:-1] * B, pay, flow
        self.dst = win_off[flow] + before.reshape(-1)                # where each payload must land
        if shuffled:
            buf = np.argsort(splitmix64(DATA_SEED ^ SHUFFLE_STREAM, nf), kind="stable").astype(np.int64)
            pool = torch.empty_like(arena)
            d_buf = torch.from_numpy(buf).to(dev)
            rows, prow = arena[:nf * B].view(nf, B), pool[:nf * B].view(nf, B)
            for i in range(0, nf, step):
                prow[d_buf[i:i + step]] = rows[i:i + step]
            self.pool = pool
        else:
            buf, self.pool = np.arange(nf, dtype=np.int64), arena
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
        self.d_buf_idx = t(buf, np.uint32).view(torch.int32)
        self.d_len16 = t(length, np.uint16)
        self.d_blk_first = t(first[:-1:64], np.uint32).view(torch.int32)
        keys = [(bytes([10, 1, f >> 8, f & 0xFF]), 40000 + f % 20000, 80) for f in range(n_flows)]
        table = rx_flow_table(keys)
        self.table_bytes = int(table.size)
        self.d_table = torch.from_numpy(table).to(dev)
        self.d_next_seq = t(next_seq, np.uint32).view(torch.int32)
        self.d_win_off = t(win_off, np.int64)
        self.d_win_len = t(win_len, np.uint32).view(torch.int32)
        self.stream = torch.zeros(self.pay_total + 16, dtype=torch.uint8, device=dev)
        self.status = torch.empty(n, dtype=torch.uint8, device=dev)
        self.l4_sum = torch.empty(n, dtype=torch.uint16, device=dev)
        self.meta = torch.empty((n, 24), dtype=torch.uint8, device=dev)


def bench_rx_place(shape, dev, args, shuffled):
    """TCP receive placement next to (a) the pool receive verify of the same pool and (b) that verify
    plus a plain device-to-device copy of the payload bytes (the floor of a two-pass design on
    payloads that were already contiguous), in alternating rounds."""
    from rustnetworkstack_amd.batch import rx_tcp_place_pool, rx_verify_pool
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6
    n = args.place_n or (1 << 20 if shape == "bulk" else 1 << 23)
    rb = RxPlaceBatch(shape, dev, n, args.place_flows, shuffled)
    st_v, l4_v = torch.empty_like(rb.status), torch.empty_like(rb.l4_sum)
    src = torch.empty(rb.pay_total, dtype=torch.uint8, device=dev)
    place = lambda: rx_tcp_place_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6,  # noqa: E731
                                      rb.d_table, rb.d_next_seq, rb.d_win_off, rb.d_win_len, rb.stream,
                                      status=rb.status, l4_sum=rb.l4_sum, meta=rb.meta)
    verify = lambda: rx_verify_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6,  # noqa: E731
                                    status=st_v, l4_sum=l4_v)

    def verify_copy():
        verify()
        rb.stream[:rb.pay_total].copy_(src)

    place()
    verify()
    torch.cuda.synchronize()
    m = rb.meta[:, 23]                                               # the place byte of every record
    placed = int((m == 7).sum().item())
    acks = int((m == 3).sum().item())
    equal = bool(torch.equal(rb.status, st_v)) and bool(torch.equal(rb.l4_sum.view(torch.int16), l4_v.view(torch.int16)))
    # the placed bytes, on a sample of datagrams (all of their bytes)
    pick = np.random.default_rng(1).choice(rb.n, min(rb.n, 4096), replace=False)
    pick = pick[rb.pay[pick] > 0]
    ok = True
    for i in pick[:512]:
        a, d, ln = int(rb.flat_off[i]) + rb.HEAD, int(rb.dst[i]), int(rb.pay[i])
        ok = ok and bool(torch.equal(rb.flat[a:a + ln], rb.stream[d:d + ln]))
    rs_p, rs_v, rs_c = timed_rounds([place, verify, verify_copy], args.steps, args.rounds)
    nf, nfl = rb.n_frags, rb.n_flows
    desc_v = 4 * nf + 2 * n + 4 * ((n + 63) // 64)

    def row(rs, desc_bytes, read_bytes, written_bytes):
        ms = rs[len(rs) // 2]
        return {"us": round(ms * 1e3, 1), "datagrams": n, "fragments": nf, "flows": nfl,
                "rounds_us": [round(x * 1e3, 1) for x in rs], "spread_us": round((rs[-1] - rs[0]) * 1e3, 1),
                "descriptor_bytes": desc_bytes, "descriptor_bytes_per_datagram": round(desc_bytes / n, 2),
                "read_bytes_per_datagram": round(read_bytes / n, 1),
                "written_bytes_per_datagram": round(written_bytes / n, 1)}

    tag = f"rx_place_{shape}" + ("_shuffled" if shuffled else "")
    tcp = placed + acks
    res = {tag: row(rs_p, desc_v + 16 * nfl + rb.table_bytes,
                    rb.total_bytes + n + tcp * rb.HEAD + rb.pay_total, 27 * n + rb.pay_total),
           tag + "_verify_only": row(rs_v, desc_v, rb.total_bytes, 3 * n),
           tag + "_verify_plus_copy": row(rs_c, desc_v, rb.total_bytes + rb.pay_total, 3 * n + rb.pay_total)}
    pr = res[tag]
    pr["placed"], pr["pure_acks"], pr["payload_bytes"] = placed, acks, rb.pay_total
    pr["status_and_l4_equal_verify"] = equal
    pr["sampled_payloads_in_place"] = ok
    med = [r[len(r) // 2] for r in (rs_p, rs_v, rs_c)]
    pr["decode_lookup_copy_us"] = round((med[0] - med[1]) * 1e3, 1)
    pr["ratio_to_verify_plus_copy"] = round(med[0] / med[2], 4)
    del rb, src
    torch.cuda.empty_cache()
    return res


def _flow_templates(nfl, dev):
    """One IPv4 template head per flow (local -> 10.1.x.y, the ports of RxPlaceBatch's flows), 64 bytes apart."""
    from rustnetworkstack_amd.workloads import LOCAL4
    f = np.arange(nfl)
    t = np.zeros((nfl, 64), dtype=np.uint8)
    t[:, 0], t[:, 8], t[:, 9] = 0x45, 64, 6
    t[:, 12:16] = np.frombuffer(LOCAL4, dtype=np.uint8)
    t[:, 16], t[:, 17], t[:, 18], t[:, 19] = 10, 1, (f >> 8) & 0xFF, f & 0xFF
    sport = 40000 + (f % 20000)
    t[:, 20], t[:, 21], t[:, 22], t[:, 23] = 0, 80, sport >> 8, sport & 0xFF
    t[:, 32] = 0x50
    return torch.from_numpy(t).to(dev), torch.full((nfl,), 40, dtype=torch.uint8, device=dev)


def _flow_rows(n, nfl, rs, names):
    med = {k: r[len(r) // 2] for k, r in zip(names, rs)}
    out = {k + "_us": round(v * 1e3, 1) for k, v in med.items()}
    out.update({k + "_rounds_us": [round(x * 1e3, 1) for x in r] for k, r in zip(names, rs)})
    out["datagrams"], out["flows"] = n, nfl
    return out, med


def bench_rx_flow(shape, dev, args):
    """The flow update and the ACK build behind the placement (see the module docstring)."""
    from rustnetworkstack_amd import _lib
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE, flow_update_work, rx_tcp_flow_update, tx_ack_build
    from rustnetworkstack_amd.batch import rx_tcp_place_pool
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6
    n = args.place_n or (1 << 20 if shape == "bulk" else 1 << 23)
    nfl = args.place_flows
    rb = RxPlaceBatch(shape, dev, n, nfl, False)
    place = lambda: rx_tcp_place_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6,  # noqa: E731
                                      rb.d_table, rb.d_next_seq, rb.d_win_off, rb.d_win_len, rb.stream,
                                      status=rb.status, l4_sum=rb.l4_sum, meta=rb.meta)
    place()
    chunk = min(n, nfl * _lib.RNS_FLOW_MAX_SEGS)                     # datagram i is flow i % nfl's: 1024 per flow and slice
    slices = [(a, min(n, a + chunk)) for a in range(0, n, chunk)]
    fl0 = np.zeros(nfl, dtype=FLOW_DTYPE)
    fl0["rcv_nxt"] = fl0["rcv_max"] = rb.d_next_seq.cpu().numpy().view(np.uint32)
    fl0["snd_wl1"], fl0["state"] = (fl0["rcv_nxt"] - 1) & 0xFFFFFFFF, _lib.RNS_TCP_ESTABLISHED
    d_fl = [torch.from_numpy(fl0.view(np.uint8)).to(dev)] + [torch.empty(nfl * 40, dtype=torch.uint8, device=dev)
                                                            for _ in range(2)]
    cap = 4
    d_pd = [torch.zeros(nfl * cap * 2, dtype=torch.int32, device=dev) for _ in range(3)]
    seg = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    res = torch.empty((len(slices), nfl, 24), dtype=torch.uint8, device=dev)
    work = torch.empty(flow_update_work(chunk, nfl), dtype=torch.uint8, device=dev)
    tmpl, hl8 = _flow_templates(nfl, dev)
    ack_cap = chunk // 5 + nfl
    out = torch.empty((ack_cap, 64), dtype=torch.uint8, device=dev)
    src, ln8 = torch.empty(ack_cap, dtype=torch.int32, device=dev), torch.empty(ack_cap, dtype=torch.uint8, device=dev)
    n_acks = torch.empty((len(slices), 2), dtype=torch.int32, device=dev)
    meta = rb.meta.reshape(-1)

    def io(k):                                                       # slice k reads state k's, writes state k + 1's
        return (0 if k == 0 else 1 + (k - 1) % 2), 1 + k % 2

    def update():
        for k, (a, b) in enumerate(slices):
            i, o = io(k)
            rx_tcp_flow_update(meta[24 * a:24 * b], d_fl[i], d_pd[i], pend_cap=cap, flows_out=d_fl[o], pend_out=d_pd[o],
                               seg=seg[a:b].reshape(-1), res=res[k].reshape(-1), work=work)

    def build():
        for k, (a, b) in enumerate(slices):
            tx_ack_build(meta[24 * a:24 * b], seg[a:b].reshape(-1), d_fl[io(k)[1]], tmpl, hl8, 1, ack_cap=ack_cap, out=out,
                         ack_src=src, ack_len8=ln8, n_acks=n_acks[k], work=work)

    def both():
        for k, (a, b) in enumerate(slices):
            i, o = io(k)
            rx_tcp_flow_update(meta[24 * a:24 * b], d_fl[i], d_pd[i], pend_cap=cap, flows_out=d_fl[o], pend_out=d_pd[o],
                               seg=seg[a:b].reshape(-1), res=res[k].reshape(-1), work=work)
            tx_ack_build(meta[24 * a:24 * b], seg[a:b].reshape(-1), d_fl[o], tmpl, hl8, 1, ack_cap=ack_cap, out=out,
                         ack_src=src, ack_len8=ln8, n_acks=n_acks[k], work=work)

    def all3():
        place()
        both()

    both()
    torch.cuda.synchronize()
    r = res.cpu().numpy().reshape(-1).view(RES_DTYPE)
    acks = n_acks.cpu().numpy()
    names = ("place", "update", "build", "all")
    row, med = _flow_rows(n, nfl, timed_rounds([place, update, build, all3], args.steps, args.rounds), names)
    added = med["all"] - med["place"]
    row.update({"slices": len(slices), "consumed": int(r["consumed"].sum()), "stopped_flows": int((r["why"] != 0).sum()),
                "readable_bytes": int(r["readable"].astype(np.int64).sum()), "payload_bytes": rb.pay_total,
                "acks": int(acks[:, 0].sum()), "acks_written_last_slice": int(min(ack_cap, acks[-1, 0])),
                "added_us": round(added * 1e3, 1), "added_ratio_to_place": round(added / med["place"], 4),
                "record_floor_bytes": 32 * n, "added_GBps_of_floor": round(32 * n / added / 1e6, 1),
                "update_GBps_of_floor": round(32 * n / med["update"] / 1e6, 1)})
    del rb
    torch.cuda.empty_cache()
    return {f"rx_flow_{shape}": row}


def bench_rx_flow_wide(dev, args, nfl=1 << 20):
    """2^20 flows, one in-order 1460-byte segment each (synthetic records, the flows in a shuffled order):
    the update and the build alone."""
    from rustnetworkstack_amd import _lib
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE, flow_update_work, rx_tcp_flow_update, tx_ack_build
    from rustnetworkstack_amd.place import META_DTYPE
    order = np.random.default_rng(20).permutation(nfl).astype(np.uint32)
    m = np.zeros(nfl, dtype=META_DTYPE)
    m["flow"], m["seq"], m["pay_len"], m["flags"], m["ip_hdr"], m["tcp_hdr"], m["place"] = order, 7 * order, 1460, 0x18, 20, 20, 7
    fl = np.zeros(nfl, dtype=FLOW_DTYPE)
    f = np.arange(nfl, dtype=np.uint32)
    fl["rcv_nxt"] = fl["rcv_max"] = 7 * f
    fl["delayed_acks"], fl["state"] = f % 5, _lib.RNS_TCP_ESTABLISHED
    t = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)  # noqa: E731
    meta, d_fl = t(m), t(fl)
    fl_out, seg = torch.empty_like(d_fl), torch.empty(nfl * 8, dtype=torch.uint8, device=dev)
    res = torch.empty(nfl * 24, dtype=torch.uint8, device=dev)
    work = torch.empty(flow_update_work(nfl, nfl), dtype=torch.uint8, device=dev)
    tmpl, hl8 = _flow_templates(nfl, dev)
    ack_cap = nfl // 4
    out = torch.empty((ack_cap, 64), dtype=torch.uint8, device=dev)
    src, ln8 = torch.empty(ack_cap, dtype=torch.int32, device=dev), torch.empty(ack_cap, dtype=torch.uint8, device=dev)
    n_acks = torch.empty(2, dtype=torch.int32, device=dev)
    update = lambda: rx_tcp_flow_update(meta, d_fl, None, pend_cap=0, flows_out=fl_out, seg=seg, res=res, work=work)  # noqa: E731
    build = lambda: tx_ack_build(meta, seg, fl_out, tmpl, hl8, 1, ack_cap=ack_cap, out=out, ack_src=src, ack_len8=ln8,  # noqa: E731
                                 n_acks=n_acks, work=work)
    update()
    build()
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(RES_DTYPE)
    row, med = _flow_rows(nfl, nfl, timed_rounds([update, build], args.steps, args.rounds), ("update", "build"))
    row.update({"consumed": int(r["consumed"].sum()), "acks": int(n_acks[0].item()),
                "update_GBps_of_floor": round(32 * nfl / med["update"] / 1e6, 1)})
    return {"rx_flow_1M_flows_x1": row}


def _conn_sample_check(m, fl, cap, got_fl, got_ctl, got_res, flows):
    """The device's out records of the flows `flows` (and their datagrams' control records) against conn_update_host
    over those flows' datagrams alone."""
    from rustnetworkstack_amd.conn import CTL_DTYPE, conn_update_host
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE
    flows = np.asarray(flows)
    idx = np.flatnonzero(np.isin(m["flow"], flows))
    sub = m[idx].copy()
    sub["flow"] = np.searchsorted(flows, sub["flow"])
    w_fl, _, w_ctl, w_res = conn_update_host(sub, fl[flows], np.zeros((len(flows), cap, 2), np.uint32) if cap else None, cap)
    g_ctl = got_ctl.cpu().numpy().reshape(-1).view(CTL_DTYPE)[idx].copy()
    g_ctl["flow"] = np.where(g_ctl["act"] != 0, np.searchsorted(flows, g_ctl["flow"]), 0)
    g_res = got_res.cpu().numpy().reshape(-1).view(RES_DTYPE)[flows].copy()
    stop = g_res["stop"] != 0xFFFFFFFF
    g_res["stop"][stop] = np.searchsorted(idx, g_res["stop"][stop])
    assert got_fl.cpu().numpy().reshape(-1).view(FLOW_DTYPE)[flows].tobytes() == w_fl.tobytes(), "rx_conn: flows differ from conn_update_host"
    assert g_ctl.tobytes() == w_ctl.tobytes() and g_res.tobytes() == w_res.tobytes(), "rx_conn: records differ from conn_update_host"


def bench_rx_conn_bulk(dev, args):
    """rx_flow's bulk shape behind the placement, through the flow update and the connection update."""
    from rustnetworkstack_amd import _lib
    from rustnetworkstack_amd.batch import rx_tcp_place_pool
    from rustnetworkstack_amd.conn import rx_tcp_conn_update
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE, flow_update_work, rx_tcp_flow_update
    from rustnetworkstack_amd.place import META_DTYPE
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6
    n, nfl, cap = args.place_n or 1 << 20, args.place_flows, 4
    rb = RxPlaceBatch("bulk", dev, n, nfl, False)
    rx_tcp_place_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6, rb.d_table, rb.d_next_seq, rb.d_win_off,
                      rb.d_win_len, rb.stream, status=rb.status, l4_sum=rb.l4_sum, meta=rb.meta)
    chunk = min(n, nfl * _lib.RNS_FLOW_MAX_SEGS)
    meta = rb.meta.reshape(-1)[:24 * chunk]
    fl0 = np.zeros(nfl, dtype=FLOW_DTYPE)
    fl0["rcv_nxt"] = fl0["rcv_max"] = rb.d_next_seq.cpu().numpy().view(np.uint32)
    fl0["snd_wl1"], fl0["state"] = (fl0["rcv_nxt"] - 1) & 0xFFFFFFFF, _lib.RNS_TCP_ESTABLISHED
    d_fl = torch.from_numpy(fl0.view(np.uint8)).to(dev)
    d_pd = torch.zeros(nfl * cap * 2, dtype=torch.int32, device=dev)
    outs = [(torch.empty_like(d_fl), torch.empty_like(d_pd), torch.empty(chunk * w, dtype=torch.uint8, device=dev),
             torch.empty(nfl * 24, dtype=torch.uint8, device=dev)) for w in (8, 16)]
    work = torch.empty(flow_update_work(chunk, nfl), dtype=torch.uint8, device=dev)
    flow = lambda: rx_tcp_flow_update(meta, d_fl, d_pd, pend_cap=cap, flows_out=outs[0][0], pend_out=outs[0][1],  # noqa: E731
                                      seg=outs[0][2], res=outs[0][3], work=work)
    conn = lambda: rx_tcp_conn_update(meta, d_fl, d_pd, pend_cap=cap, flows_out=outs[1][0], pend_out=outs[1][1],  # noqa: E731
                                      ctl=outs[1][2], res=outs[1][3], work=work)
    flow()
    conn()
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][3], outs[1][3]), "rx_conn: the two updates differ"
    _conn_sample_check(meta.cpu().numpy().view(META_DTYPE), fl0, cap, outs[1][0], outs[1][2], outs[1][3], [0, 1, nfl - 1])
    r = outs[1][3].cpu().numpy().view(RES_DTYPE)
    row, med = _flow_rows(chunk, nfl, timed_rounds([flow, conn], args.steps, args.rounds), ("flow_update", "conn_update"))
    row.update({"consumed": int(r["consumed"].sum()), "sends": int(r["n_acks"].sum()),
                "conn_over_flow": round(med["conn_update"] / med["flow_update"], 4)})
    del rb
    torch.cuda.empty_cache()
    return {"rx_conn_bulk": row}


def _conn_wide(dev, args, nfl, state, pay, flags, both, name):
    from rustnetworkstack_amd.conn import rx_tcp_conn_update
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE, flow_update_work, rx_tcp_flow_update
    from rustnetworkstack_amd.place import META_DTYPE
    order = np.random.default_rng(20).permutation(nfl).astype(np.uint32)
    m = np.zeros(nfl, dtype=META_DTYPE)
    m["flow"], m["seq"], m["pay_len"], m["flags"], m["ip_hdr"], m["tcp_hdr"] = order, 7 * order, pay, flags, 20, 20
    m["ack"], m["place"] = 5 * order + 1, 7 if pay else 3
    fl = np.zeros(nfl, dtype=FLOW_DTYPE)
    f = np.arange(nfl, dtype=np.uint32)
    fl["rcv_nxt"] = fl["rcv_max"] = 7 * f
    fl["snd_nxt"], fl["snd_una"], fl["snd_wl1"] = 5 * f, 7 * f - 1, 7 * f - 1
    fl["delayed_acks"], fl["state"] = f % 5, state
    t = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)  # noqa: E731
    meta, d_fl = t(m), t(fl)
    outs = [(torch.empty_like(d_fl), torch.empty(nfl * w, dtype=torch.uint8, device=dev), torch.empty(nfl * 24, dtype=torch.uint8, device=dev))
            for w in (8, 16)]
    work = torch.empty(flow_update_work(nfl, nfl), dtype=torch.uint8, device=dev)
    flow = lambda: rx_tcp_flow_update(meta, d_fl, None, pend_cap=0, flows_out=outs[0][0], seg=outs[0][1], res=outs[0][2], work=work)  # noqa: E731
    conn = lambda: rx_tcp_conn_update(meta, d_fl, None, pend_cap=0, flows_out=outs[1][0], ctl=outs[1][1], res=outs[1][2], work=work)  # noqa: E731
    conn()
    torch.cuda.synchronize()
    _conn_sample_check(m, fl, 0, outs[1][0], outs[1][1], outs[1][2], np.arange(0, nfl, nfl // 997))
    fns, names = ([flow, conn], ("flow_update", "conn_update")) if both else ([conn], ("conn_update",))
    if both:
        flow()
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2]), "rx_conn: the two updates differ"
    r = outs[1][2].cpu().numpy().view(RES_DTYPE)
    row, med = _flow_rows(nfl, nfl, timed_rounds(fns, args.steps, args.rounds), names)
    st = outs[1][0].cpu().numpy().view(FLOW_DTYPE)["state"]
    row.update({"consumed": int(r["consumed"].sum()), "sends": int(r["n_acks"].sum()), "states": np.bincount(st, minlength=11).tolist(),
                "update_GBps_of_floor": round((24 + 16 + 80 + 24) * nfl / med["conn_update"] / 1e6, 1)})
    if both:
        row["conn_over_flow"] = round(med["conn_update"] / med["flow_update"], 4)
    return {name: row}


def bench_rx_conn_wide(dev, args, nfl=1 << 20):
    """rx_flow's 2^20-flows shape (one in-order 1460-byte segment each) through both updates."""
    from rustnetworkstack_amd import _lib
    return _conn_wide(dev, args, nfl, _lib.RNS_TCP_ESTABLISHED, 1460, 0x18, True, "rx_conn_1M_flows_x1")


def bench_rx_conn_handshake(dev, args, nfl=1 << 20):
    """2^20 SynReceived flows, each with its handshake-completing ACK: the lane path."""
    from rustnetworkstack_amd import _lib
    return _conn_wide(dev, args, nfl, _lib.RNS_TCP_SYN_RECEIVED, 0, 0x10, False, "rx_conn_1M_handshakes")


def bench_rx_conn_lifecycle(dev, args, nfl=1 << 18):
    """2^18 connections: ACK, request, FIN|ACK in one call, then our close and the last ACK in a second, and the control build."""
    from rustnetworkstack_amd import _lib
    from rustnetworkstack_amd.conn import CTL_DTYPE, rx_tcp_conn_update, tx_tcp_close, tx_tcp_ctl_build
    from rustnetworkstack_amd.flow import FLOW_DTYPE, RES_DTYPE, flow_update_work
    from rustnetworkstack_amd.place import META_DTYPE
    rng = np.random.default_rng(21)
    f = np.arange(nfl, dtype=np.uint32)
    fl = np.zeros(nfl, dtype=FLOW_DTYPE)
    fl["rcv_nxt"] = fl["rcv_max"] = 11 * f + 1
    fl["snd_una"], fl["snd_nxt"], fl["snd_wl1"], fl["state"] = 11 * f, 3 * f, 11 * f, _lib.RNS_TCP_SYN_RECEIVED
    slot = np.repeat(f, 3)
    rng.shuffle(slot)                                                   # the connections interleaved; a flow's own order kept
    rank = np.zeros(3 * nfl, dtype=np.int64)
    o = np.argsort(slot, kind="stable")
    rank[o] = np.tile(np.arange(3), nfl)
    m = np.zeros(3 * nfl, dtype=META_DTYPE)
    m["flow"], m["ack"], m["ip_hdr"], m["tcp_hdr"], m["window"] = slot, 3 * slot + 1, 20, 20, 0x2000
    m["seq"] = 11 * slot + 1 + np.where(rank == 2, 100, 0)
    m["pay_len"], m["flags"] = np.where(rank == 1, 100, 0), np.choose(rank, [0x10, 0x18, 0x11])
    m["place"] = np.where(rank == 1, 7, 3)
    m2 = np.zeros(nfl, dtype=META_DTYPE)
    o2 = rng.permutation(nfl).astype(np.uint32)
    m2["flow"], m2["seq"], m2["ack"], m2["flags"], m2["ip_hdr"], m2["tcp_hdr"], m2["place"] = o2, 11 * o2 + 102, 3 * o2 + 2, 0x10, 20, 20, 3
    t = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)  # noqa: E731
    d_m, d_m2, d_fl = t(m), t(m2), t(fl)
    fl1, fl2, fl3 = (torch.empty_like(d_fl) for _ in range(3))
    ctl1, ctl2 = torch.empty(3 * nfl * 16, dtype=torch.uint8, device=dev), torch.empty(nfl * 16, dtype=torch.uint8, device=dev)
    cctl = torch.empty(nfl * 16, dtype=torch.uint8, device=dev)
    res1, res2 = (torch.empty(nfl * 24, dtype=torch.uint8, device=dev) for _ in range(2))
    op = torch.ones(nfl, dtype=torch.uint8, device=dev)
    work = torch.empty(flow_update_work(3 * nfl, nfl), dtype=torch.uint8, device=dev)
    tmpl, hl8 = _flow_templates(nfl, dev)
    out = torch.empty((nfl, 64), dtype=torch.uint8, device=dev)
    src, ln8 = torch.empty(nfl, dtype=torch.int32, device=dev), torch.empty(nfl, dtype=torch.uint8, device=dev)
    cnt = torch.empty(2, dtype=torch.int32, device=dev)
    first = lambda: rx_tcp_conn_update(d_m, d_fl, None, pend_cap=0, flows_out=fl1, ctl=ctl1, res=res1, work=work)  # noqa: E731
    close = lambda: tx_tcp_close(fl1, op, flows_out=fl2, ctl=cctl)  # noqa: E731
    build = lambda: tx_tcp_ctl_build(cctl, nfl, tmpl, hl8, 1, out_cap=nfl, out=out, src=src, len8=ln8, count=cnt, work=work)  # noqa: E731
    last = lambda: rx_tcp_conn_update(d_m2, fl2, None, pend_cap=0, flows_out=fl3, ctl=ctl2, res=res2, work=work)  # noqa: E731

    def whole():
        first()
        close()
        build()
        last()

    whole()
    torch.cuda.synchronize()
    sample = np.arange(0, nfl, nfl // 499)
    _conn_sample_check(m, fl, 0, fl1, ctl1, res1, sample)
    _conn_sample_check(m2, fl2.cpu().numpy().view(FLOW_DTYPE), 0, fl3, ctl2, res2, sample)
    st = fl3.cpu().numpy().view(FLOW_DTYPE)["state"]
    assert (st == _lib.RNS_TCP_CLOSED).all() and int(cnt[0].item()) == nfl, "rx_conn: the lifecycle did not close every connection"
    assert (cctl.cpu().numpy().view(CTL_DTYPE)["flags"] == 0x11).all()
    r1 = res1.cpu().numpy().view(RES_DTYPE)
    row, med = _flow_rows(4 * nfl, nfl, timed_rounds([first, close, build, last, whole], args.steps, args.rounds),
                          ("update_3seg", "close", "ctl_build", "update_last_ack", "whole"))
    row.update({"consumed": int(r1["consumed"].sum()) + nfl, "sends_first_call": int(r1["n_acks"].sum()), "fins_built": int(cnt[0].item()),
                "whole_Msegs_per_s": round(4 * nfl / med["whole"] / 1e3, 1)})
    return {"rx_conn_256k_lifecycles": row}


def bench_tx_plan(nfl, k, dev, args, mss=1460):
    """The send planner in front of the segmentation offload (see the module docstring): nfl flows, k whole
    segments queued each."""
    from rustnetworkstack_amd import _lib
    from rustnetworkstack_amd.batch import _stream_handle, fill_splitmix64
    from rustnetworkstack_amd.flow import FLOW_DTYPE
    from rustnetworkstack_amd.segment import tx_segment_layout
    from rustnetworkstack_amd.send import RES_DTYPE, tx_plan_work
    n, E, per = nfl * k, 2 * nfl, k * mss
    head_first = (nfl * per + 15) // 16 * 16
    arena = torch.empty(head_first + 40 * n + 64, dtype=torch.uint8, device=dev)
    fill_splitmix64(arena, 0x5E9D)
    f = np.arange(nfl, dtype=np.uint64)
    fl = np.zeros(nfl, dtype=FLOW_DTYPE)
    fl["snd_una"] = fl["snd_nxt"] = (0x1000 + 77777 * f) & 0xFFFFFFFF
    fl["snd_wnd"], fl["rcv_nxt"], fl["rq_len"], fl["state"] = 0xFFFF, (5 + 3 * f) & 0xFFFFFFFF, f & 0xFFF, _lib.RNS_TCP_ESTABLISHED
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_fl, d_fl_out = t(fl.view(np.uint8)), torch.empty(nfl * 40, dtype=torch.uint8, device=dev)
    d_sq_off, d_sq_seq = t((f * per).view(np.int64)), t(fl["snd_una"].view(np.int32))
    d_sq_len, d_mss = t(np.full(nfl, per, dtype=np.int32)), t(np.full(nfl, mss, dtype=np.uint16))
    tmpl, hl8 = _flow_templates(nfl, dev)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    o = {"tmpl": new((E, 64), torch.uint8), "hl8": new(E, torch.uint8), "pay_off": new(E, torch.int64), "pay_len": new(E, torch.int32),
         "mss": new(E, torch.uint16), "head_off": new(E, torch.int64), "seg_first": new(E + 1, torch.int32),
         "blk_flow": new((n + 63) // 64, torch.int32), "n": new(2, torch.int32), "res": new(nfl * 16, torch.uint8)}
    work = new(tx_plan_work(nfl), torch.uint8)
    status, status_a = new(n, torch.uint8), new(n, torch.uint8)
    # (a)'s descriptors: the host's layout over the flows, the templates patched as send_packet fills them
    th = tmpl.cpu().numpy().copy()
    be = lambda v, nb: np.stack([(v >> (8 * (nb - 1 - i))) & 0xFF for i in range(nb)], axis=1).astype(np.uint8)  # noqa: E731
    th[:, 4:6] = be((7 + f * k) & 0xFFFF, 2)
    th[:, 24:28], th[:, 28:32] = be(fl["snd_nxt"].astype(np.uint64), 4), be(fl["rcv_nxt"].astype(np.uint64), 4)
    th[:, 32], th[:, 33] = 0x50, 0x18
    th[:, 34:36] = be((0xFFFF - (fl["rq_len"].astype(np.uint64) & 0xFFFF)) & 0xFFFF, 2)
    sf, ho, bf, n_seg, _ = tx_segment_layout(np.full(nfl, per), np.full(nfl, mss), np.full(nfl, 40), head_first)
    assert n_seg == n
    a = {"tmpl": t(th), "pay_off": d_sq_off, "pay_len": d_sq_len, "mss": d_mss, "head_off": t(ho.view(np.int64)),
         "seg_first": t(sf.view(np.int32)), "blk_flow": t(bf.view(np.int32))}
    lib, st = _lib.load(), _stream_handle(dev)
    p = lambda x: x.data_ptr()  # noqa: E731
    seg_a_args = (p(arena), arena.numel(), p(a["tmpl"]), 64, p(hl8), p(a["pay_off"]), p(a["pay_len"]), p(a["mss"]),
                  p(a["head_off"]), p(a["seg_first"]), p(a["blk_flow"]), nfl, n, p(status_a), st)
    seg_b_args = (p(arena), arena.numel(), p(o["tmpl"]), 64, p(o["hl8"]), p(o["pay_off"]), p(o["pay_len"]), p(o["mss"]),
                  p(o["head_off"]), p(o["seg_first"]), p(o["blk_flow"]), E, n, p(status), st)
    plan_args = (p(d_fl), p(d_fl_out), nfl, p(d_sq_off), p(d_sq_seq), p(d_sq_len), p(d_mss), None, p(tmpl), 64, p(hl8), 7, None,
                 head_first, n, p(o["tmpl"]), p(o["hl8"]), p(o["pay_off"]), p(o["pay_len"]), p(o["mss"]), p(o["head_off"]),
                 p(o["seg_first"]), p(o["blk_flow"]), p(o["n"]), p(o["res"]), p(work), work.numel(), st)

    def seg_alone():
        _lib.check(lib.rns_tx_segment_dev(*seg_a_args), "rns_tx_segment_dev")

    def plan():
        _lib.check(lib.rns_tx_tcp_plan_dev(*plan_args), "rns_tx_tcp_plan_dev")

    def both():
        plan()
        _lib.check(lib.rns_tx_segment_dev(*seg_b_args), "rns_tx_segment_dev")

    seg_alone()
    heads_a = arena[head_first:head_first + 40 * n].clone()
    arena[head_first:head_first + 40 * n] = 0
    both()
    torch.cuda.synchronize()
    res = o["res"].cpu().numpy().view(RES_DTYPE)
    same = bool(torch.equal(heads_a, arena[head_first:head_first + 40 * n]))
    filled = int((status == 3).sum().item())
    names = ("segment", "plan_segment", "plan")
    row, med = _flow_rows(n, nfl, timed_rounds([seg_alone, both, plan], args.steps, args.rounds), names)
    row.update({k2 + "_spread_us": round(row[k2 + "_rounds_us"][-1] - row[k2 + "_rounds_us"][0], 1) for k2 in names})
    row.update({"segments_planned": int(o["n"][0].item()), "new_bytes": int(res["new_bytes"].astype(np.int64).sum()),
                "filled": filled, "heads_equal_host_layout": same, "payload_bytes": n * mss,
                "added_us": round((med["plan_segment"] - med["segment"]) * 1e3, 1),
                "added_ratio_to_segment": round((med["plan_segment"] - med["segment"]) / med["segment"], 4)})
    del arena, heads_a
    torch.cuda.empty_cache()
    return {f"tx_plan_{nfl}_flows_x{k}": row}


def _be_words(rows):
    """Per row: the folded sum of its big-endian 16-bit words (int64 tensor)."""
    s = rows[:, 0::2].sum(dim=1, dtype=torch.int64) * 256 + rows[:, 1::2].sum(dim=1, dtype=torch.int64)
    for _ in range(3):
        s = (s & 0xFFFF) + (s >> 16)
    return s


def _echo_batch(shape, n, dev, B=512):
    """n datagrams from 192.168.1.1 to L4 in a pool of B-byte buffers, built on the device: every one an
    IPv4 ping (ping84, ping1500), or IMIX sizes with every fourth a ping and the others UDP.  Datagram i
    lies in consecutive buffers from i * stride on, zeros after its end.  (pool, buf_idx, blk_first, len16
    as device tensors; the lengths and the request mask as numpy.)"""
    from rustnetworkstack_amd.batch import rx_pool_layout
    i = np.arange(n)
    if shape == "imix":
        T = np.where(i % 12 < 7, 40, np.where(i % 12 < 11, 576, 1500)).astype(np.int64)
        req = i % 4 == 0
    else:
        T = np.full(n, int(shape[4:]), dtype=np.int64)
        req = np.ones(n, dtype=bool)
    stride = int(-(-int(T.max()) // B))
    W = stride * B
    blk, first, nf = rx_pool_layout(T, B)
    nfr = -(-T // B)
    idx = (np.repeat(i * stride, nfr) + (np.arange(nf) - np.repeat(first[:-1].astype(np.int64), nfr))).astype(np.uint32)
    pool = torch.zeros(n * W, dtype=torch.uint8, device=dev)
    rows = pool.view(n, W)
    Tt, reqt = torch.from_numpy(T).to(dev), torch.from_numpy(req).to(dev)
    col = torch.arange(W, device=dev)
    for lo in range(0, n, 1 << 18):  # the payloads: random bytes inside the datagram, zeros after it
        hi = min(n, lo + (1 << 18))
        rnd = torch.randint(0, 256, (hi - lo, W), dtype=torch.uint8, device=dev)
        rows[lo:hi] = rnd * (col[None, :] < Tt[lo:hi, None]).to(torch.uint8)
        del rnd
    hdr = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
    hdr[:, 0], hdr[:, 8] = 0x45, 64
    hdr[:, 2], hdr[:, 3] = (Tt >> 8).to(torch.uint8), (Tt & 255).to(torch.uint8)
    hdr[:, 9] = torch.where(reqt, 1, 17).to(torch.uint8)
    hdr[:, 12:16] = torch.tensor([192, 168, 1, 1], dtype=torch.uint8, device=dev)
    hdr[:, 16:20] = torch.tensor(list(L4), dtype=torch.uint8, device=dev)
    ck = 0xFFFF ^ _be_words(hdr[:, :20])
    hdr[:, 10], hdr[:, 11] = (ck >> 8).to(torch.uint8), (ck & 255).to(torch.uint8)
    hdr[:, 20] = 8  # echo request, code 0, checksum below (UDP: these are its port bytes)
    rows[:, :24] = hdr
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        ck = 0xFFFF ^ _be_words(rows[lo:hi, 20:])
        rows[lo:hi, 22], rows[lo:hi, 23] = (ck >> 8).to(torch.uint8), (ck & 255).to(torch.uint8)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)  # noqa: E731
    return pool, dv(idx, np.int32), dv(blk, np.int32), dv(T.astype(np.uint16), np.int16), T, req


def bench_rx_echo(shape, dev, args, B=512):
    """rns_rx_icmp_echo_pool_dev against the pool verify alone and against the verify followed by
    rns_tx_fill_pool_dev over prebuilt replies of the same shapes (the floor that copies nothing), in
    alternating rounds."""
    from rustnetworkstack_amd.batch import echo_host, echo_work, rx_icmp_echo_pool, rx_verify_pool, tx_fill_pool
    n = args.echo_n or (1 << 23 if shape == "imix" else 1 << 20)
    pool, idx, blk, len16, T, req = _echo_batch(shape, n, dev, B)
    nreq, pay = int(req.sum()), T[req] - 24
    nbuf = int((1 + -(-pay // B)).sum())
    rng = np.random.default_rng(15)
    free_h = rng.permutation(nbuf).astype(np.uint32)
    free = torch.from_numpy(free_h.view(np.int32)).to(dev)
    tx = torch.zeros(nbuf * B, dtype=torch.uint8, device=dev)
    keep = dict(status=torch.empty(n, dtype=torch.uint8, device=dev), echo=torch.empty(n, dtype=torch.uint8, device=dev),
                tx_blk_first=torch.empty((nreq + 63) // 64, dtype=torch.int32, device=dev),
                tx_head_len8=torch.empty(nreq, dtype=torch.uint8, device=dev),
                tx_pay_len16=torch.empty(nreq, dtype=torch.uint16, device=dev), tx_src=torch.empty(nreq, dtype=torch.int32, device=dev),
                count=torch.empty(3, dtype=torch.int32, device=dev),
                work=torch.empty((echo_work(n) + 7) // 8, dtype=torch.int64, device=dev))

    def echo():
        rx_icmp_echo_pool(pool, idx, blk, len16, L4, L6, tx, free, buf_bytes=B, reply_cap=nreq, ip_id_base=1, **keep)

    echo()
    torch.cuda.synchronize()
    cnt = keep["count"].cpu().numpy().view(np.uint32)
    assert cnt.tolist() == [nreq, nbuf, nreq], cnt
    assert int((keep["echo"] == 3).sum().item()) == nreq
    # a sample against the host path: the first 256 datagrams' replies, byte for byte
    m = 256
    W = pool.numel() // n
    small = int(-(-T[:m] // B).sum())
    k = int((1 + -(-(T[:m][req[:m]] - 24) // B)).sum())
    txh = np.zeros(k * B, dtype=np.uint8)
    e = echo_host(pool[:m * W].cpu().numpy(), idx[:small].cpu().numpy().view(np.uint32), blk[:m // 64].cpu().numpy().view(np.uint32),
                  T[:m].astype(np.uint16), L4, L6, txh, np.arange(k, dtype=np.uint32), buf_bytes=B, ip_id_base=1)
    got = tx.view(-1, B)[torch.from_numpy(free_h[:k].astype(np.int64)).to(dev)].cpu().numpy()
    want, nb = txh.reshape(-1, B), 0
    for hl, pl in zip(e[4].tolist(), e[5].tolist()):  # the head's bytes and the payload's, not the slack after them
        npay = -(-pl // B)
        assert np.array_equal(got[nb, B - hl:], want[nb, B - hl:])
        assert np.array_equal(got[nb + 1:nb + 1 + npay].reshape(-1)[:pl], want[nb + 1:nb + 1 + npay].reshape(-1)[:pl])
        nb += 1 + npay
    assert nb == k
    st2 = torch.empty(n, dtype=torch.uint8, device=dev)
    tst = torch.empty(nreq, dtype=torch.uint8, device=dev)

    def verify():
        rx_verify_pool(pool, idx, blk, len16, L4, L6, buf_bytes=B, status=st2)

    def verify_fill():
        verify()
        tx_fill_pool(tx, free, keep["tx_blk_first"], keep["tx_head_len8"], keep["tx_pay_len16"], buf_bytes=B, status=tst)

    verify_fill()
    torch.cuda.synchronize()
    assert int((tst == 3).sum().item()) == nreq and torch.equal(st2, keep["status"])
    rs = timed_rounds([echo, verify, verify_fill], args.steps, args.rounds)
    med = [r[len(r) // 2] for r in rs]
    rx_bytes, pay_bytes = int(T.sum()), int(pay.sum())
    row = {"datagrams": n, "requests": nreq, "reply_buffers": nbuf, "rx_bytes": rx_bytes, "payload_bytes": pay_bytes,
           "echo_us": round(med[0] * 1e3, 1), "verify_us": round(med[1] * 1e3, 1), "verify_fill_us": round(med[2] * 1e3, 1),
           "echo_over_verify": round(med[0] / med[1], 3), "echo_over_verify_fill": round(med[0] / med[2], 3),
           "added_us_per_copied_GB": round((med[0] - med[1]) * 1e3 / max(pay_bytes / 1e9, 1e-9), 1),
           "echo_GBps_rx_plus_copied": round((rx_bytes + 2 * pay_bytes) / med[0] / 1e6, 1),
           "rounds_us": {k: [round(x * 1e3, 1) for x in r] for k, r in zip(("echo", "verify", "verify_fill"), rs)}}
    del pool, tx
    torch.cuda.empty_cache()
    return {f"rx_echo_{shape}": row}


def _udp_batch(shape, n, n_socks, dev, B=512):
    """n UDP datagrams from 192.168.1.1 to L4 in a pool of B-byte buffers, built on the device: all of one
    length (udp1500, udp64) or IMIX lengths; datagram i goes to socket (7919 i) mod n_socks, whose port is
    1024 + 3 s, and lies in consecutive buffers from i * stride on, zeros after its end.  (pool, buf_idx,
    blk_first, len16 as device tensors; the lengths, the sockets and the ports as numpy.)"""
    from rustnetworkstack_amd.batch import rx_pool_layout
    from rustnetworkstack_amd.workloads import DATA_SEED, imix_lengths
    i = np.arange(n)
    T = imix_lengths(n, DATA_SEED).astype(np.int64) if shape == "imix" else np.full(n, int(shape[3:]), dtype=np.int64)
    sock = (i * 7919) % n_socks
    ports = 1024 + 3 * np.arange(n_socks)
    stride = int(-(-int(T.max()) // B))
    W = stride * B
    blk, first, nf = rx_pool_layout(T, B)
    nfr = -(-T // B)
    idx = (np.repeat(i * stride, nfr) + (np.arange(nf) - np.repeat(first[:-1].astype(np.int64), nfr))).astype(np.uint32)
    pool = torch.zeros(n * W, dtype=torch.uint8, device=dev)
    rows = pool.view(n, W)
    Tt = torch.from_numpy(T).to(dev)
    col = torch.arange(W, device=dev)
    for lo in range(0, n, 1 << 18):  # the payloads: random bytes inside the datagram, zeros after it
        hi = min(n, lo + (1 << 18))
        rnd = torch.randint(0, 256, (hi - lo, W), dtype=torch.uint8, device=dev)
        rows[lo:hi] = rnd * (col[None, :] < Tt[lo:hi, None]).to(torch.uint8)
        del rnd
    dport = torch.from_numpy(ports[sock]).to(dev)
    hdr = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
    hdr[:, 0], hdr[:, 8], hdr[:, 9] = 0x45, 64, 17
    hdr[:, 2], hdr[:, 3] = (Tt >> 8).to(torch.uint8), (Tt & 255).to(torch.uint8)
    hdr[:, 12:16] = torch.tensor([192, 168, 1, 1], dtype=torch.uint8, device=dev)
    hdr[:, 16:20] = torch.tensor(list(L4), dtype=torch.uint8, device=dev)
    ck = 0xFFFF ^ _be_words(hdr[:, :20])
    hdr[:, 10], hdr[:, 11] = (ck >> 8).to(torch.uint8), (ck & 255).to(torch.uint8)
    hdr[:, 20], hdr[:, 21] = 0x9C, 0x40  # source port 40000
    hdr[:, 22], hdr[:, 23] = (dport >> 8).to(torch.uint8), (dport & 255).to(torch.uint8)
    hdr[:, 24], hdr[:, 25] = ((Tt - 20) >> 8).to(torch.uint8), ((Tt - 20) & 255).to(torch.uint8)
    rows[:, :28] = hdr
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)  # noqa: E731
    return pool, dv(idx, np.int32), dv(blk, np.int32), dv(T.astype(np.uint16), np.int16), T, sock, ports, nf


def bench_rx_udp(shape, n_socks, dev, args, B=512):
    """rns_rx_udp_demux_pool_dev against the pool verify alone and against the TCP placement of RxPlaceBatch's
    segments of the same datagram sizes, in alternating rounds."""
    from rustnetworkstack_amd.batch import demux_work, port_table, rx_tcp_place_pool, rx_udp_demux_pool, rx_verify_pool
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6
    n = args.udp_n or (1 << 23 if shape == "imix" else 1 << 20)
    pool, idx, blk, len16, T, sock, ports, nf = _udp_batch(shape, n, n_socks, dev, B)
    pay = T - 28
    units = -(-pay // 16)
    tbl = torch.from_numpy(port_table(ports).view(np.int16)).to(dev)
    keep = dict(status=torch.empty(n, dtype=torch.uint8, device=dev), udp=torch.empty(n, dtype=torch.uint8, device=dev),
                pos=torch.empty(n, dtype=torch.int32, device=dev), rec=torch.empty(32 * n, dtype=torch.uint8, device=dev),
                data=torch.empty(16 * int(units.sum()) + 16, dtype=torch.uint8, device=dev),
                q_first=torch.empty(n_socks + 1, dtype=torch.int32, device=dev), count=torch.empty(2, dtype=torch.int32, device=dev),
                work=torch.empty((demux_work(n, n_socks) + 15) // 8, dtype=torch.int64, device=dev))

    def demux():
        rx_udp_demux_pool(pool, idx, blk, len16, L4, L6, tbl, n_socks, buf_bytes=B, **keep)

    demux()
    torch.cuda.synchronize()
    cnt = keep["count"].cpu().numpy().view(np.uint32)
    assert cnt.tolist() == [n, int(units.sum())], cnt
    assert int((keep["udp"] == 7).sum().item()) == n
    qf = np.concatenate([[0], np.cumsum(np.bincount(sock, minlength=n_socks))])
    assert np.array_equal(keep["q_first"].cpu().numpy().view(np.uint32), qf)
    # a sample against the pool: the record's fields and the payload, byte for byte
    W = pool.numel() // n
    posh = keep["pos"].cpu().numpy().view(np.uint32)
    for i in np.random.default_rng(16).choice(n, 256, replace=False).tolist():
        k = int(posh[i])
        r = keep["rec"][32 * k:32 * k + 32].cpu().numpy()
        src, off16, sport, ln = (int(r[16:20].view(np.uint32)[0]), int(r[20:24].view(np.uint32)[0]), int(r[24:26].view(np.uint16)[0]),
                                 int(r[26:28].view(np.uint16)[0]))
        assert qf[sock[i]] <= k < qf[sock[i] + 1] and (src, sport, ln, r[28], r[29]) == (i, 40000, int(pay[i]), 4, 7)
        assert bytes(r[:16]) == bytes([192, 168, 1, 1]) + bytes(12)
        assert torch.equal(keep["data"][16 * off16:16 * off16 + ln], pool[i * W + 28:i * W + 28 + ln])
    st2 = torch.empty(n, dtype=torch.uint8, device=dev)

    def verify():
        rx_verify_pool(pool, idx, blk, len16, L4, L6, buf_bytes=B, status=st2)

    verify()
    torch.cuda.synchronize()
    assert torch.equal(st2, keep["status"])
    fns, names, rb = [demux, verify], ["demux", "verify"], None
    if shape != "udp64":
        rb = RxPlaceBatch("bulk" if shape == "udp1500" else "imix", dev, n, 1024, False)
        fns.append(lambda: rx_tcp_place_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6, rb.d_table,
                                             rb.d_next_seq, rb.d_win_off, rb.d_win_len, rb.stream, status=rb.status,
                                             l4_sum=rb.l4_sum, meta=rb.meta))
        names.append("place")
    rs = timed_rounds(fns, args.steps, args.rounds)
    med = [r[len(r) // 2] for r in rs]
    rx_bytes, pay_bytes = int(T.sum()), int(pay.sum())
    row = {"datagrams": n, "sockets": n_socks, "fragments": nf, "rx_bytes": rx_bytes, "payload_bytes": pay_bytes,
           "work_bytes": demux_work(n, n_socks), "demux_us": round(med[0] * 1e3, 1), "verify_us": round(med[1] * 1e3, 1),
           "demux_over_verify": round(med[0] / med[1], 3),
           "added_us_per_copied_GB": round((med[0] - med[1]) * 1e3 / max(pay_bytes / 1e9, 1e-9), 1),
           "demux_GBps_rx_plus_copied": round((rx_bytes + 2 * pay_bytes) / med[0] / 1e6, 1),
           "rounds_us": {k: [round(x * 1e3, 1) for x in r] for k, r in zip(names, rs)}}
    if rb is not None:
        row.update({"place_us": round(med[2] * 1e3, 1), "place_payload_bytes": rb.pay_total,
                    "demux_over_place": round(med[0] / med[2], 3),
                    "place_added_us_per_copied_GB": round((med[2] - med[1]) * 1e3 / max(rb.pay_total / 1e9, 1e-9), 1)})
    del pool, keep, rb
    torch.cuda.empty_cache()
    return {f"rx_udp_{shape}_{n_socks}": row}


def bench_tx_udp(shape, n_socks, dev, args, B=512):
    """rns_tx_udp_send_pool_dev over the demux's own output — an echo server's sends — against
    rns_tx_fill_pool_dev over the datagrams it built (the floor that copies nothing), the demux followed by the
    send build against the demux alone, and a plain device copy of the payload bytes, in alternating rounds."""
    from rustnetworkstack_amd.batch import (demux_work, port_table, rx_udp_demux_pool, send_host, tx_fill_pool, tx_udp_send_pool,
                                            udp_send_work)
    n = args.udp_n or (1 << 23 if shape == "imix" else 1 << 20)
    rx_shape = shape if shape == "imix" else f"udp{int(shape[3:]) + 28}"  # the received datagram: 28 bytes of headers more
    pool, idx, blk, len16, T, sock, ports, nf = _udp_batch(rx_shape, n, n_socks, dev, B)
    pay = T - 28
    units = -(-pay // 16)
    tbl = torch.from_numpy(port_table(ports).view(np.int16)).to(dev)
    dm = dict(status=torch.empty(n, dtype=torch.uint8, device=dev), udp=torch.empty(n, dtype=torch.uint8, device=dev),
              pos=torch.empty(n, dtype=torch.int32, device=dev), rec=torch.zeros(32 * n, dtype=torch.uint8, device=dev),
              data=torch.empty(16 * int(units.sum()) + 16, dtype=torch.uint8, device=dev),
              q_first=torch.empty(n_socks + 1, dtype=torch.int32, device=dev), count=torch.empty(2, dtype=torch.int32, device=dev),
              work=torch.empty((demux_work(n, n_socks) + 15) // 8, dtype=torch.int64, device=dev))

    def demux():
        rx_udp_demux_pool(pool, idx, blk, len16, L4, L6, tbl, n_socks, buf_bytes=B, **dm)

    demux()
    nbuf = int((1 + -(-pay // B)).sum())
    free_h = np.random.default_rng(18).permutation(nbuf).astype(np.uint32)
    free = torch.from_numpy(free_h.view(np.int32)).to(dev)
    tx = torch.zeros(nbuf * B, dtype=torch.uint8, device=dev)
    d_ports = torch.from_numpy(ports.astype(np.uint16).view(np.int16)).to(dev)
    keep = dict(send=torch.empty(n, dtype=torch.uint8, device=dev), tx_blk_first=torch.empty((n + 63) // 64, dtype=torch.int32, device=dev),
                tx_head_len8=torch.empty(n, dtype=torch.uint8, device=dev), tx_pay_len16=torch.empty(n, dtype=torch.uint16, device=dev),
                tx_src=torch.empty(n, dtype=torch.int32, device=dev), count=torch.empty(3, dtype=torch.int32, device=dev),
                work=torch.empty((udp_send_work(n) + 7) // 8, dtype=torch.int64, device=dev))

    def send():
        tx_udp_send_pool(dm["data"], dm["rec"], dm["q_first"], d_ports, L4, L6, tx, free, buf_bytes=B, ip_id_base=1, **keep)

    send()
    torch.cuda.synchronize()
    cnt = keep["count"].cpu().numpy().view(np.uint32)
    assert cnt.tolist() == [n, nbuf, n], cnt
    assert int((keep["send"] == 3).sum().item()) == n
    # a sample against the host path: the first 256 records' datagrams, byte for byte
    m = 256
    rec_h = dm["rec"][:32 * m].cpu().numpy()
    from rustnetworkstack_amd.udp import REC
    r256 = rec_h.view(REC)
    end = int((r256["off16"].astype(np.int64) + -(-r256["len"].astype(np.int64) // 16)).max())
    k = int((1 + -(-r256["len"].astype(np.int64) // B)).sum())
    txh = np.zeros(k * B, dtype=np.uint8)
    qh = np.minimum(dm["q_first"].cpu().numpy().view(np.uint32), m)
    e = send_host(dm["data"][:16 * end].cpu().numpy(), r256, qh, ports, L4, L6, txh, np.arange(k, dtype=np.uint32), buf_bytes=B, ip_id_base=1)
    assert int(e.count[0]) == m and int(e.count[1]) == k
    got = tx.view(-1, B)[torch.from_numpy(free_h[:k].astype(np.int64)).to(dev)].cpu().numpy()
    want, nb = txh.reshape(-1, B), 0
    for hl, pl in zip(e.tx_head_len8.tolist(), e.tx_pay_len16.tolist()):  # the head's bytes and the payload's, not the slack after them
        npay = -(-pl // B)
        assert np.array_equal(got[nb, B - hl:], want[nb, B - hl:])
        assert np.array_equal(got[nb + 1:nb + 1 + npay].reshape(-1)[:pl], want[nb + 1:nb + 1 + npay].reshape(-1)[:pl])
        nb += 1 + npay
    assert nb == k
    tst = torch.empty(n, dtype=torch.uint8, device=dev)

    def fill():
        tx_fill_pool(tx, free, keep["tx_blk_first"], keep["tx_head_len8"], keep["tx_pay_len16"], buf_bytes=B, status=tst)

    fill()
    torch.cuda.synchronize()
    assert int((tst == 3).sum().item()) == n

    def demux_send():
        demux()
        send()

    pay_bytes = int(pay.sum())
    src_copy = dm["data"][:pay_bytes]
    dst_copy = torch.empty(pay_bytes, dtype=torch.uint8, device=dev)

    def copy():
        dst_copy.copy_(src_copy)

    names = ("send", "fill", "demux_send", "demux", "copy")
    rs = timed_rounds([send, fill, demux_send, demux, copy], args.steps, args.rounds)
    med = [r[len(r) // 2] for r in rs]
    row = {"sends": n, "sockets": n_socks, "tx_buffers": nbuf, "payload_bytes": pay_bytes, "work_bytes": udp_send_work(n),
           "send_us": round(med[0] * 1e3, 1), "fill_us": round(med[1] * 1e3, 1), "demux_send_us": round(med[2] * 1e3, 1),
           "demux_us": round(med[3] * 1e3, 1), "copy_us": round(med[4] * 1e3, 1),
           "send_over_fill": round(med[0] / med[1], 3), "send_over_copy": round(med[0] / med[4], 3),
           "demux_send_minus_demux_us": round((med[2] - med[3]) * 1e3, 1),
           "send_GBps_read_plus_written": round((2 * pay_bytes + 32 * n + (28 + 7) * n) / med[0] / 1e6, 1),
           "rounds_us": {k: [round(x * 1e3, 1) for x in r] for k, r in zip(names, rs)}}
    del pool, dm, keep, tx, dst_copy
    torch.cuda.empty_cache()
    return {f"tx_udp_{shape}_{n_socks}": row}


def _listen_batch(shape, n, dev):
    """The rx_listen op's batch as an RxPlaceBatch whose pool the placement reads: syn — 44-byte IPv4 SYNs with an MSS
    option from distinct sources to port 80; stray — 40-byte pure ACKs from distinct sources; imix — RxPlaceBatch's imix
    over 1024 flows, of which every hundredth datagram is a SYN from a source of its own and the one after it a stray."""
    from rustnetworkstack_amd.workloads import LOCAL4
    B = RxPlaceBatch.BUF
    if shape == "imix":
        rb = RxPlaceBatch("imix", dev, n, 1024, False)
        who = torch.arange(0, n, 100, device=dev)
        for k, flags in ((0, 0x02), (1, 0x10)):                      # a SYN, then a stray ACK, each from 10.(2 + k).x.y:p
            i = who + k
            i = i[i < n]
            at = torch.from_numpy(rb.flat_off).to(dev)[i]
            src = i // 100
            rb.pool[at + 13] = 2 + k
            rb.pool[at + 14] = ((src >> 8) & 0xFF).to(torch.uint8)
            rb.pool[at + 15] = (src & 0xFF).to(torch.uint8)
            rb.pool[at + 20] = (4 + (src >> 16)).to(torch.uint8)     # the source port's high byte: more sources than 2^16
            rb.pool[at + 33] = flags
        length = torch.from_numpy(rb.d_len16.cpu().numpy().astype(np.int32)).to(dev)
        st = tx_fill(rb.pool, torch.from_numpy(rb.flat_off).to(dev), length)
        assert int((st != 3).sum().item()) == 0
        return rb, (n + 99) // 100, (n + 98) // 100
    H = 44 if shape == "syn" else 40
    rb = RxPlaceBatch.__new__(RxPlaceBatch)
    from rustnetworkstack_amd.batch import rx_flow_table
    i = np.arange(n)
    h = np.zeros((n, B), dtype=np.uint8)
    h[:, 0], h[:, 3], h[:, 6], h[:, 8], h[:, 9] = 0x45, H, 0x40, 64, 6
    h[:, 12], h[:, 13], h[:, 14], h[:, 15] = 10, 2 + (i >> 16), (i >> 8) & 0xFF, i & 0xFF
    h[:, 16:20] = np.frombuffer(LOCAL4, dtype=np.uint8)
    h[:, 20], h[:, 21], h[:, 23] = 0x90, i & 0xFF, 80
    h[:, 24:28] = np.stack([(i >> 16) & 0xFF, (i >> 8) & 0xFF, i & 0xFF, 7 * i & 0xFF], axis=1)
    h[:, 32], h[:, 33], h[:, 34] = (H - 20) << 2, 0x02 if shape == "syn" else 0x10, 0x20
    if shape == "syn":
        h[:, 40:44] = [2, 4, 0x05, 0xB4]
    rb.pool = torch.from_numpy(h.reshape(-1)).to(dev)
    rb.flat_off = i.astype(np.int64) * B
    st = tx_fill(rb.pool, torch.from_numpy(rb.flat_off).to(dev), torch.full((n,), H, dtype=torch.int32, device=dev))
    assert int((st != 3).sum().item()) == 0
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
    rb.n, rb.n_flows, rb.n_frags = n, 1024, n
    rb.d_buf_idx, rb.d_len16 = t(i, np.uint32).view(torch.int32), t(np.full(n, H), np.uint16)
    rb.d_blk_first = t(i[::64], np.uint32).view(torch.int32)
    rb.d_table = torch.from_numpy(rx_flow_table([(bytes([10, 1, f >> 8, f & 0xFF]), 40000 + f, 80) for f in range(1024)])).to(dev)
    rb.d_next_seq = torch.zeros(1024, dtype=torch.int32, device=dev)
    rb.d_win_off, rb.d_win_len = torch.zeros(1024, dtype=torch.int64, device=dev), torch.zeros(1024, dtype=torch.int32, device=dev)
    rb.stream = torch.zeros(16, dtype=torch.uint8, device=dev)
    rb.status, rb.l4_sum = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint16, device=dev)
    rb.meta = torch.empty((n, 24), dtype=torch.uint8, device=dev)
    return rb, (n if shape == "syn" else 0), (0 if shape == "syn" else n)


def bench_rx_listen(shape, dev, args):
    """rns_rx_tcp_listen_pool_dev behind the placement, against verify + placement alone (the launches it follows) and
    against rns_tx_ack_build_dev over the same number of heads (the floor that classifies nothing), in alternating
    rounds; counts and a sample of replies and accept records compared with listen_host before timing."""
    from rustnetworkstack_amd.batch import listen_host, listen_work, port_table, rx_tcp_listen_pool, rx_tcp_place_pool
    from rustnetworkstack_amd.flow import FLOW_DTYPE, SEG_DTYPE, flow_update_work, tx_ack_build
    from rustnetworkstack_amd.listen import ACCEPT_DTYPE
    from rustnetworkstack_amd.place import meta_records
    from rustnetworkstack_amd.workloads import LOCAL4, LOCAL6
    n = args.listen_n or (1 << 23 if shape == "imix" else 1 << 20)
    rb, syns, strays = _listen_batch(shape, n, dev)
    replies = syns + strays
    place = lambda: rx_tcp_place_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6,  # noqa: E731
                                      rb.d_table, rb.d_next_seq, rb.d_win_off, rb.d_win_len, rb.stream,
                                      status=rb.status, l4_sum=rb.l4_sum, meta=rb.meta)
    place()
    tbl = torch.from_numpy(port_table([80]).view(np.int16)).to(dev)
    iss = torch.arange(1, replies + 1, dtype=torch.int32, device=dev)
    keep = dict(out=torch.empty(64 * replies, dtype=torch.uint8, device=dev), rep_src=torch.empty(replies, dtype=torch.int32, device=dev),
                rep_len8=torch.empty(replies, dtype=torch.uint8, device=dev),
                accept=torch.empty(72 * replies, dtype=torch.uint8, device=dev), count=torch.empty(3, dtype=torch.int32, device=dev),
                conn=torch.empty(n, dtype=torch.uint8, device=dev),
                work=torch.empty((listen_work(n) + 7) // 8, dtype=torch.int64, device=dev))
    meta = rb.meta.reshape(-1)

    def listen():
        rx_tcp_listen_pool(rb.pool, rb.d_buf_idx, rb.d_blk_first, rb.d_len16, LOCAL4, LOCAL6, meta, tbl, 1, iss, reply_cap=replies,
                           ip_id_base=1, **keep)

    listen()
    torch.cuda.synchronize()
    cnt = keep["count"].cpu().numpy().view(np.uint32)
    assert cnt.tolist() == [replies, replies, syns], (cnt, replies, syns)
    # a sample against the host path: the first 4096 datagrams' replies and accept records, byte for byte
    m = min(n, 4096)
    nfh = int(rb.d_blk_first[m // 64].item()) if m < n else rb.n_frags
    e = listen_host(rb.pool[:nfh * rb.BUF].cpu().numpy(), rb.d_buf_idx[:nfh].cpu().numpy().view(np.uint32),
                    rb.d_blk_first[:m // 64].cpu().numpy().view(np.uint32), rb.d_len16[:m].cpu().numpy(), LOCAL4, LOCAL6,
                    meta_records(rb.meta[:m]), port_table([80]), 1, np.arange(1, m + 1), ip_id_base=1)
    R, A = int(e.count[0]), int(e.count[2])
    assert R > 0 and np.array_equal(keep["conn"][:m].cpu().numpy(), e.conn)
    lens = keep["rep_len8"][:R].cpu().numpy().astype(np.int64)
    got = keep["out"][:64 * R].cpu().numpy().reshape(R, 64)
    assert np.array_equal(lens, e.rep_len8[:R]) and all(np.array_equal(got[k, :lens[k]], e.out[64 * k:64 * k + lens[k]]) for k in range(R))
    assert keep["accept"][:72 * A].cpu().numpy().tobytes() == e.accept[:A].tobytes() and ACCEPT_DTYPE.itemsize == 72
    # the floor: the ACK build over as many heads, one flow's template, nothing classified
    seg_h = np.zeros(n, dtype=SEG_DTYPE)
    conn_h = keep["conn"].cpu().numpy()
    seg_h["act"][(conn_h & 0x0A) != 0] = 2                           # an ACK where the responder answers
    d_seg = torch.from_numpy(seg_h.view(np.uint8)).to(dev)
    fmeta = rb.meta.clone().reshape(-1)
    fmeta.view(torch.int32).reshape(n, 6)[:, 0] = 0                  # every ACK is flow 0's
    tmpl, hl8 = _flow_templates(1, dev)
    fl = torch.from_numpy(np.zeros(1, dtype=FLOW_DTYPE).view(np.uint8)).to(dev)
    ak = dict(out=torch.empty((replies, 64), dtype=torch.uint8, device=dev), ack_src=torch.empty(replies, dtype=torch.int32, device=dev),
              ack_len8=torch.empty(replies, dtype=torch.uint8, device=dev), n_acks=torch.empty(2, dtype=torch.int32, device=dev),
              work=torch.empty(flow_update_work(n, 0), dtype=torch.uint8, device=dev))

    def acks():
        tx_ack_build(fmeta, d_seg, fl, tmpl, hl8, 1, ack_cap=replies, **ak)

    acks()
    torch.cuda.synchronize()
    assert ak["n_acks"].cpu().numpy().tolist() == [replies, replies]

    def place_listen():
        place()
        listen()

    names = ("listen", "place", "place_listen", "ack_floor")
    rs = timed_rounds([listen, place, place_listen, acks], args.steps, args.rounds)
    med = [r[len(r) // 2] for r in rs]
    row = {"datagrams": n, "syns": syns, "strays": strays, "replies": replies, "work_bytes": listen_work(n),
           "listen_us": round(med[0] * 1e3, 1), "place_us": round(med[1] * 1e3, 1), "place_listen_us": round(med[2] * 1e3, 1),
           "ack_floor_us": round(med[3] * 1e3, 1), "added_us": round((med[2] - med[1]) * 1e3, 1),
           "added_ratio_to_place": round((med[2] - med[1]) / med[1], 4), "listen_over_ack_floor": round(med[0] / med[3], 3),
           "rounds_us": {k: [round(x * 1e3, 1) for x in r] for k, r in zip(names, rs)}}
    del rb, keep, ak, fmeta
    torch.cuda.empty_cache()
    return {f"rx_listen_{shape}": row}


def bench_chain_netbuf(lay, dev, args, shuffled=False, runs=False):
    """Fragments as NetBuffer holds them: packet i of L bytes is ceil(L/512) fragments,
    each in its own 512-byte buffer (buf.rs:50; the fragment arena is those buffers
    back to back, filled with splitmix64 bytes).  shuffled: fragment f lives in buffer
    perm[f] (a random permutation), as buffers from a free list are."""
    from rustnetworkstack_amd.batch import fill_splitmix64
    n, pay = lay.n, lay.payload_bytes
    L = lay.length.astype(np.int64)
    nfr = (L + 511) // 512
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nfr, out=first[1:])
    nf = int(first[-1])
    pkt = np.repeat(np.arange(n), nfr)
    k = np.arange(nf) - first[:-1][pkt]
    slot = np.random.default_rng(0x5B0F).permutation(nf) if shuffled else np.arange(nf)
    frag_off = slot.astype(np.uint64) * np.uint64(512)
    frag_len = np.minimum(L[pkt] - 512 * k, 512).astype(np.uint32)
    arena = torch.empty(nf * 512 + 16, dtype=torch.uint8, device=dev)
    fill_splitmix64(arena, 0xF4A6)
    d_fo = torch.from_numpy(frag_off.view(np.int64)).to(dev)
    d_fl = torch.from_numpy(frag_len.view(np.int32)).to(dev)
    d_first = torch.from_numpy(first.astype(np.uint32).view(np.int32)).to(dev)
    seed = torch.from_numpy(lay.seed.view(np.int16)).to(dev)
    out = torch.empty(n, dtype=torch.uint16, device=dev)
    ms = timed(lambda: csum_chain(arena, d_fo, d_fl, d_first, seed, complement=True, out=out,
                                  frag_len_hint=int(round(pay / nf)), runs=runs),
               args.steps, args.rounds)
    del arena
    torch.cuda.empty_cache()
    return {"us": round(ms * 1e3, 1), "GBps": round((pay + 2 * n) / ms / 1e6, 1), "fragments": nf,
            "layout": "netbuf: 512-byte fragment buffers" + (", shuffled" if shuffled else ", in order")}


if __name__ == "__main__":
    main()
