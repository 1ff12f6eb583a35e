/*
 * A plain C caller of TCP send planning (rns_tx_tcp_plan_dev, rns_tx_tcp_plan_work) followed by the
 * segmentation offload (rns_tx_segment_dev) on the planned descriptors, bound the way the reference's
 * Rust would bind them (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for
 * device memory.  40 flows (IPv4 and IPv6 alternating, some not Established, some with nothing to
 * send, some behind a closed window, every third with its retransmit timer fired) are planned on the
 * device; every output array is checked against tcp_write's loop (tcp.rs:256-292), retransmit
 * (tcp.rs:329-348) and send_packet (tcp.rs:402-447) restated here piece by piece, and after the
 * segmentation — launched with n_seg = seg_cap, nothing read back in between — every arena byte and
 * status against oracle_tx_chain_fill (oracle/csum_oracle.c, linked as test infrastructure only) on
 * the chains the pieces expand to.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x91A45EEDull
#include "abi_test.h"

enum { NFL = 40, E = 2 * NFL, STRIDE = 64, SEGCAP = 1000, NBLK = (SEGCAP + 63) / 64, SQ = 20000, DATA = NFL * (SQ + 1) + 64,
       ARENA = DATA + SEGCAP * 60 + 64, FILL = 0xEE, IDBASE = 0xFFF0, IDADD = 7 };

int main(void)
{
    static rns_tcp_flow flow[NFL], flow_out[NFL], w_flow[NFL];
    static rns_tx_plan_res res[NFL], w_res[NFL];
    static uint64_t sq_off[NFL], pay_off[E], head_off[E], w_pay_off[E], w_head_off[E], frag_off[2 * SEGCAP];
    static uint32_t sq_seq[NFL], sq_len[NFL], pay_len[E], seg_first[E + 1], blk_flow[NBLK], n_out[2], w_pay_len[E], w_seg_first[E + 1],
        w_blk_flow[NBLK], frag_len[2 * SEGCAP], first[SEGCAP + 1];
    static uint16_t mss[NFL], mss_out[E];
    static uint8_t rexmit[NFL], hl8[NFL], tmpl[NFL * STRIDE], tmpl_out[E * STRIDE], w_tmpl[E * STRIDE], hl8_out[E], arena[ARENA],
        want[ARENA], back[ARENA], status[SEGCAP], w_status[SEGCAP];
    const uint64_t head_first = DATA;

    fill_random_bytes(arena, ARENA);
    for (uint32_t f = 0; f < NFL; ++f) {
        rns_tcp_flow *s = &flow[f];
        const uint32_t inflight = f % 4 == 1 ? 0 : (uint32_t)(next_u64() % 4000), acked = (uint32_t)(next_u64() % 500);
        const uint32_t unsent = f % 7 == 3 ? 0 : (uint32_t)(next_u64() % 12000);
        s->snd_una = f == 5 ? 0xFFFFFF00u : (uint32_t)next_u64();  /* one across 2^32 */
        s->snd_nxt = s->snd_una + inflight;
        s->snd_wnd = f % 9 == 4 ? 0 : (uint32_t)(next_u64() % 16000);
        s->rcv_nxt = (uint32_t)next_u64();
        s->rcv_max = s->rcv_nxt;
        s->rq_len = f % 5 == 0 ? 0x10000u + f : (uint32_t)(next_u64() % 0xffff);
        s->snd_wl1 = f; s->snd_wl2 = 2 * f; s->n_pend = f % 3; s->delayed_acks = (uint16_t)(f % 5); s->ack_timer = f & 1;
        s->state = f % 11 == 6 ? 4 : RNS_TCP_ESTABLISHED;
        sq_seq[f] = s->snd_una - acked;
        sq_len[f] = acked + inflight + unsent;
        sq_off[f] = 33 + (uint64_t)f * (SQ + 1);  /* any byte alignment */
        mss[f] = (uint16_t)(f % 6 == 2 ? 100 + f : 1460);
        rexmit[f] = f % 3 == 0;
        uint8_t *t = tmpl + f * STRIDE;
        fill_random_bytes(t, STRIDE);
        if (f & 1) {
            hl8[f] = 60; t[0] = 0x60; t[6] = 6; t[7] = 64; t[52] = 0x50;
        } else {
            hl8[f] = 40; t[0] = 0x45; t[6] = 0x40; t[7] = 0; t[8] = 64; t[9] = 6; t[32] = 0x50;
        }
        if (f == 20)
            t[32] = 0x70;  /* a data offset the planner does not take */
    }

    /* the expected plan: the reference's loops, piece by piece */
    memset(w_tmpl, FILL, sizeof w_tmpl);
    memcpy(want, arena, ARENA);
    for (uint32_t b = 0; b < NBLK; ++b)
        w_blk_flow[b] = E;
    uint32_t n_seg = 0, next_packet_id = (IDBASE + IDADD) & 0xffff, n_v4 = 0, n_rex = 0, n_wait = 0;
    uint64_t head_at = head_first;
    for (uint32_t f = 0; f < NFL; ++f) {
        const rns_tcp_flow *s = &flow[f];
        const uint32_t inflight = s->snd_nxt - s->snd_una, a = s->snd_una - sq_seq[f], hl = hl8[f], ip = hl == 40 ? 20 : 40;
        const uint8_t *t = tmpl + f * STRIDE;
        w_flow[f] = *s;
        memset(&w_res[f], 0, sizeof w_res[f]);
        uint32_t why = RNS_PLAN_NONE, npiece[2] = {0, 0}, nbytes[2] = {0, 0};
        if (s->state != RNS_TCP_ESTABLISHED) {
            why = RNS_PLAN_STATE;
        } else if ((t[ip + 12] >> 4) != 5) {
            why = RNS_PLAN_TMPL;
        } else {
            if (rexmit[f] && inflight) {  /* tcp.rs:338-342 */
                npiece[0] = 1;
                nbytes[0] = inflight < mss[f] ? inflight : mss[f];
            }
            uint32_t offset = 0, next_seq = s->snd_nxt;
            const uint32_t len = sq_len[f] - a - inflight;
            while (offset < len) {  /* tcp.rs:257-285 */
                const uint32_t packet_length = len - offset < mss[f] ? len - offset : mss[f];
                if (seq_gt(next_seq + packet_length, s->snd_una + s->snd_wnd)) {
                    why = RNS_PLAN_WINDOW;  /* tcp.rs:269: the wait */
                    break;
                }
                next_seq += packet_length;
                offset += packet_length;
                npiece[1] += 1;
            }
            nbytes[1] = offset;
        }
        for (uint32_t k = 0; k < 2; ++k) {
            const uint32_t e = 2 * f + k;
            w_seg_first[e] = n_seg;
            w_head_off[e] = head_at;
            w_pay_off[e] = 0;
            w_pay_len[e] = 0;
            if (!npiece[k])
                continue;
            w_pay_off[e] = sq_off[f] + a + (k ? inflight : 0);
            w_pay_len[e] = nbytes[k];
            uint8_t *row = w_tmpl + e * STRIDE;
            memcpy(row, t, hl);
            put32(row + ip + 4, s->snd_nxt);  /* send_next_seq, for the retransmit too (tcp.rs:439) */
            put32(row + ip + 8, s->rcv_nxt);
            row[ip + 12] = 0x50;
            row[ip + 13] = 0x18;
            const uint32_t window = (0xffffu - (s->rq_len & 0xffffu)) & 0xffffu;  /* tcp.rs:403 */
            put16(row + ip + 14, window);
            if (hl == 40)
                put16(row + 4, next_packet_id);
            for (uint32_t j = 0; j < npiece[k]; ++j, ++n_seg) {
                const uint32_t seglen = nbytes[k] - j * mss[f] < mss[f] ? nbytes[k] - j * mss[f] : mss[f];
                if (n_seg % 64 == 0)
                    w_blk_flow[n_seg / 64] = e;
                first[n_seg] = 2 * n_seg;
                frag_off[2 * n_seg] = head_at + (uint64_t)j * hl;
                frag_len[2 * n_seg] = hl;
                frag_off[2 * n_seg + 1] = w_pay_off[e] + (uint64_t)j * mss[f];
                frag_len[2 * n_seg + 1] = seglen;
                make_segment_head(want + frag_off[2 * n_seg], row, hl, j, mss[f], seglen);
                if (hl == 40) {  /* NEXT_PACKET_ID.fetch_add(1), ip_output_v4 only */
                    next_packet_id = (next_packet_id + 1) & 0xffff;
                    n_v4 += 1;
                }
            }
            head_at += (uint64_t)npiece[k] * hl;
            if (k == 0) {
                w_res[f].rexmit_bytes = nbytes[0];
                n_rex += 1;
            } else {
                w_res[f].new_bytes = nbytes[1];
                w_res[f].new_segs = npiece[1];
                w_flow[f].snd_nxt += nbytes[1];
            }
        }
        w_res[f].why = (uint8_t)why;
        n_wait += why == RNS_PLAN_WINDOW;
    }
    w_seg_first[E] = n_seg;
    first[n_seg] = 2 * n_seg;
    CHECK(n_seg > 100 && n_seg + 64 < SEGCAP && n_rex > 5 && n_wait > 5 && n_v4 > 0 && n_v4 < n_seg,
          "%u segments, %u retransmits, %u waiting", n_seg, n_rex, n_wait);
    oracle_tx_chain_fill(want, ARENA, frag_off, frag_len, first, 2 * n_seg, n_seg, w_status);
    for (uint32_t i = n_seg; i < SEGCAP; ++i)
        w_status[i] = RNS_TX_MALFORMED;

    /* the argument checks need no device */
    uint64_t need = 0, need2 = 0;
    CHECK(rns_tx_tcp_plan_work(NFL, &need) == RNS_OK && need >= 16 * NFL, "the workspace: %llu", (unsigned long long)need);
    CHECK(rns_tx_tcp_plan_work(NFL + 1, &need2) == RNS_OK && need2 >= need, "monotone");
    CHECK(rns_tx_tcp_plan_work(NFL, NULL) == RNS_E_INVALID && rns_tx_tcp_plan_work((1u << 30) + 1, &need2) == RNS_E_INVALID,
          "the workspace helper's checks");

    rns_tcp_flow *d_flow = NULL, *d_flow_out = NULL;
    rns_tx_plan_res *d_res = NULL;
    uint64_t *d_sq_off = NULL, *d_pay_off = NULL, *d_head_off = NULL;
    uint32_t *d_sq_seq = NULL, *d_sq_len = NULL, *d_pay_len = NULL, *d_seg_first = NULL, *d_blk_flow = NULL, *d_n = NULL, *d_add = NULL;
    uint16_t *d_mss = NULL, *d_mss_out = NULL;
    uint8_t *d_rexmit = NULL, *d_hl8 = NULL, *d_tmpl = NULL, *d_tmpl_out = NULL, *d_hl8_out = NULL, *d_arena = NULL, *d_status = NULL;
    void *d_work = NULL;
    const uint32_t add[1] = {IDADD + 0x30000u};  /* mod 2^16 */
    UP(d_flow, flow, sizeof flow);
    UP(d_sq_off, sq_off, sizeof sq_off);
    UP(d_sq_seq, sq_seq, sizeof sq_seq);
    UP(d_sq_len, sq_len, sizeof sq_len);
    UP(d_mss, mss, sizeof mss);
    UP(d_rexmit, rexmit, sizeof rexmit);
    UP(d_hl8, hl8, sizeof hl8);
    UP(d_tmpl, tmpl, sizeof tmpl);
    UP(d_add, add, sizeof add);
    UP(d_arena, arena, ARENA);
    OUT(d_flow_out, sizeof flow_out, FILL);
    OUT(d_res, sizeof res, FILL);
    OUT(d_pay_off, sizeof pay_off, FILL);
    OUT(d_head_off, sizeof head_off, FILL);
    OUT(d_pay_len, sizeof pay_len, FILL);
    OUT(d_seg_first, sizeof seg_first, FILL);
    OUT(d_blk_flow, sizeof blk_flow, FILL);
    OUT(d_n, sizeof n_out, FILL);
    OUT(d_mss_out, sizeof mss_out, FILL);
    OUT(d_tmpl_out, sizeof tmpl_out, FILL);
    OUT(d_hl8_out, sizeof hl8_out, FILL);
    OUT(d_status, sizeof status, FILL);
    OUT(d_work, need, FILL);

    CHECK(rns_tx_tcp_plan_dev(d_flow, d_flow_out, NFL, d_sq_off, d_sq_seq, d_sq_len, d_mss, d_rexmit, d_tmpl, 0, d_hl8, IDBASE, d_add,
                              head_first, SEGCAP, d_tmpl_out, d_hl8_out, d_pay_off, d_pay_len, d_mss_out, d_head_off, d_seg_first,
                              d_blk_flow, d_n, d_res, d_work, need, NULL) == RNS_E_INVALID, "tmpl_stride == 0");
    CHECK(rns_tx_tcp_plan_dev(d_flow, d_flow_out, NFL, d_sq_off, d_sq_seq, d_sq_len, d_mss, d_rexmit, d_tmpl, STRIDE, d_hl8, IDBASE,
                              d_add, head_first, SEGCAP, d_tmpl_out, d_hl8_out, d_pay_off, d_pay_len, d_mss_out, d_head_off,
                              d_seg_first, d_blk_flow, d_n, d_res, d_work, need - 1, NULL) == RNS_E_INVALID, "a short workspace");
    hipStream_t st;
    HIP_OK(abi_stream(&st));
    /* plan, then segment with n_seg = seg_cap: one stream, nothing read in between */
    int rc = rns_tx_tcp_plan_dev(d_flow, d_flow_out, NFL, d_sq_off, d_sq_seq, d_sq_len, d_mss, d_rexmit, d_tmpl, STRIDE, d_hl8, IDBASE,
                                 d_add, head_first, SEGCAP, d_tmpl_out, d_hl8_out, d_pay_off, d_pay_len, d_mss_out, d_head_off,
                                 d_seg_first, d_blk_flow, d_n, d_res, d_work, need, st);
    CHECK(rc == RNS_OK, "rns_tx_tcp_plan_dev: %d", rc);
    rc = rns_tx_segment_dev(d_arena, ARENA, d_tmpl_out, STRIDE, d_hl8_out, d_pay_off, d_pay_len, d_mss_out, d_head_off, d_seg_first,
                            d_blk_flow, E, SEGCAP, d_status, st);
    CHECK(rc == RNS_OK, "rns_tx_segment_dev: %d", rc);
    HIP_OK(hipStreamSynchronize(st));
    DOWN(flow_out, d_flow_out, sizeof flow_out);
    DOWN(res, d_res, sizeof res);
    DOWN(pay_off, d_pay_off, sizeof pay_off);
    DOWN(head_off, d_head_off, sizeof head_off);
    DOWN(pay_len, d_pay_len, sizeof pay_len);
    DOWN(seg_first, d_seg_first, sizeof seg_first);
    DOWN(blk_flow, d_blk_flow, sizeof blk_flow);
    DOWN(n_out, d_n, sizeof n_out);
    DOWN(mss_out, d_mss_out, sizeof mss_out);
    DOWN(tmpl_out, d_tmpl_out, sizeof tmpl_out);
    DOWN(hl8_out, d_hl8_out, sizeof hl8_out);
    DOWN(status, d_status, sizeof status);
    DOWN(back, d_arena, ARENA);

    CHECK(n_out[0] == n_seg && n_out[1] == n_v4, "d_n: %u, %u (want %u, %u)", n_out[0], n_out[1], n_seg, n_v4);
    CHECK(memcmp(flow_out, w_flow, sizeof flow_out) == 0, "the flow records");
    CHECK(memcmp(res, w_res, sizeof res) == 0, "the results");
    for (uint32_t f = 0; f < NFL; ++f)
        CHECK(res[f].why == w_res[f].why && res[f].new_bytes == w_res[f].new_bytes && res[f].rexmit_bytes == w_res[f].rexmit_bytes,
              "flow %u: why %u (%u), new %u (%u), rexmit %u (%u)", f, res[f].why, w_res[f].why, res[f].new_bytes, w_res[f].new_bytes,
              res[f].rexmit_bytes, w_res[f].rexmit_bytes);
    for (uint32_t e = 0; e < E; ++e) {
        CHECK(pay_off[e] == w_pay_off[e] && pay_len[e] == w_pay_len[e] && head_off[e] == w_head_off[e] &&
                  seg_first[e] == w_seg_first[e] && mss_out[e] == mss[e / 2] && hl8_out[e] == hl8[e / 2],
              "entry %u", e);
        CHECK(memcmp(tmpl_out + e * STRIDE, w_tmpl + e * STRIDE, STRIDE) == 0, "entry %u: its template row", e);
    }
    CHECK(seg_first[E] == n_seg, "seg_first[E]");
    CHECK(memcmp(blk_flow, w_blk_flow, sizeof blk_flow) == 0, "blk_flow");
    for (uint32_t i = 0; i < SEGCAP; ++i)
        CHECK(status[i] == w_status[i], "status %u: %02x != %02x", i, status[i], w_status[i]);
    for (size_t b = 0; b < ARENA; ++b)
        CHECK(back[b] == want[b], "arena byte %zu: %02x != %02x", b, back[b], want[b]);

    return abi_finish("%u segments of %u flows, %u retransmits, %u flows waiting", n_seg, NFL, n_rex, n_wait);
}
