// Batched Internet (RFC 1071) checksum for MI355X (gfx950, CDNA4).
//
// The reference computes compute_ones_comp (src/stack/util.rs:88-106) once per
// packet on whichever CPU thread handles it.  Here a batch of
// packets already resident in HBM is checksummed by one launch:
//
//   * a packet is owned by a GROUP of G lanes (G = 4..64, a power of two, so a
//     64-lane wavefront serves 64/G packets at once); the group streams the
//     packet as 16-byte aligned chunks, lane l taking chunks l, l+G, ...,
//     U chunks in flight per lane (global_load_dwordx4, fully coalesced);
//   * bytes outside [start, start+len) in the first / last chunk are masked
//     to zero, so packets may start at any byte offset and the odd final
//     byte is the zero-padded word the reference adds as byte << 8;
//   * each dword is split by two v_dot4_u32_u8 into the sum of the bytes that
//     are the HIGH half of a big-endian word and the sum of the LOW halves
//     (which is which depends on the packet start's parity).  The reference's
//     u32 accumulator is exactly  seed + 256*high + low  (mod 2^32), so the
//     per-lane u32 partials are summed with wrap-around across the group
//     (shuffle butterfly) and folded end-around exactly like util.rs:101-103:
//     bit-exact for every length, including the reference's wrap past 128 KiB;
//   * one lane per group stores the u16 result (optionally ^ 0xffff).
//
// This is a bandwidth-bound integer reduction (~1 byte of HBM per 0.5 VALU
// op): no MFMA, no LDS staging needed for the data itself.  Roofline: HBM read
// bandwidth; algorithmic bytes per packet = len + 2.
#pragma once

// The device code, by kernel family (each part includes the ones it builds on): first the byte-order
// helpers and the TCP head builder, last the scan and the arguments of the multi-launch entry points.
// rns_k_flow.hpp, rns_k_conn.hpp, rns_k_plan.hpp, rns_k_echo.hpp, rns_k_udp.hpp, rns_k_udp_tx.hpp and rns_k_listen.hpp
// hold kernels that are no templates and are not listed: k_flow.hip, k_conn.hip, k_plan.hip, k_echo.hip, k_udp.hip,
// k_udp_tx.hip and k_listen.hip, which launch them, include them (k_flow and k_conn share the lists' launches and the
// state and step blocks of rns_k_flow_step.hpp; k_conn's walk frames are rns_k_flow_walk.hpp).
#include "rns_k_tcp_head.hpp"
#include "rns_k_common.hpp"
#include "rns_k_rounds.hpp"
#include "rns_k_mixed.hpp"
#include "rns_k_chain.hpp"
#include "rns_k_chain_rx.hpp"
#include "rns_k_pool_rx.hpp"
#include "rns_k_stream.hpp"
#include "rns_k_rows.hpp"
#include "rns_k_rows_rx.hpp"
#include "rns_k_rows_tx.hpp"
#include "rns_k_txrows.hpp"
#include "rns_k_pool_tx.hpp"
#include "rns_k_segment.hpp"
#include "rns_k_pool_view.hpp"
#include "rns_k_pool_place.hpp"
#include "rns_k_scan.hpp"
#include "rns_k_pool_txform.hpp"
#include "rns_k_args.hpp"
