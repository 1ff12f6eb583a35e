/*
 * A plain C caller of TCP segmentation offload (rns_tx_segment_dev) and its host helpers
 * (rns_tx_segment_layout, rns_tx_segment_chains), bound the way the reference's Rust would bind them
 * (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for device memory.  60 sends —
 * TCP over IPv4 and IPv6, with and without TCP options, mss 1460, 537 and 1, empty sends between them,
 * data at every byte alignment, heads from an odd offset — are laid out by the helpers, segmented on
 * the device and checked, every arena byte and every status, against oracle_tx_chain_fill
 * (oracle/csum_oracle.c, linked as test infrastructure only) on a host copy whose heads a few lines of
 * C build from the templates (tcp.rs:938-976, ip.rs:140-177), over the chains the form expands to.  A
 * second round gives one send a template with a bad version: its segments alone are rejected.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x5E67F00Dull
#include "abi_test.h"

enum { NFL = 60, STRIDE = 72, MAXSEG = 4096, PAY_BYTES = 1 << 20, ARENA = PAY_BYTES + MAXSEG * STRIDE, BAD_FLOW = 30 };

/* A template head of kind k (0: IPv4, 1: IPv6, 2: IPv4 + 12 option bytes, 3: IPv6 + 12): its length.
 * The fields the device fills hold random bytes. */
static uint32_t make_template(uint8_t *t, int k, uint32_t seq, uint16_t id)
{
    const uint32_t iphdr = (k & 1) ? 40 : 20, doff = k >= 2 ? 8 : 5, hl = iphdr + 4 * doff;
    fill_random_bytes(t, hl);
    if (k & 1) {
        t[0] = 0x60; t[6] = 6; t[7] = 64;
    } else {
        t[0] = 0x45; put16(t + 4, id); t[6] = 0x40; t[7] = 0; t[8] = 64; t[9] = 6;
    }
    uint8_t *tcp = t + iphdr;
    put32(tcp + 4, seq);
    tcp[12] = (uint8_t)(doff << 4); tcp[13] = 0x18;  /* ACK | PSH */
    return hl;
}

int main(void)
{
    static uint8_t arena[ARENA], want[ARENA], back[ARENA], tmpl[NFL * STRIDE], hl8[NFL], status[MAXSEG], want_st[MAXSEG];
    static uint16_t mss[NFL];
    static uint32_t pay_len[NFL], seg_first[NFL + 1], blk_flow[(MAXSEG + 63) / 64], frag_len[2 * MAXSEG], first[MAXSEG + 1];
    static uint64_t pay_off[NFL], head_off[NFL], frag_off[2 * MAXSEG];
    fill_random_bytes(arena, sizeof arena);
    uint64_t at = 64;
    for (uint32_t f = 0; f < NFL; ++f) {
        static const uint16_t ms[] = {1460, 537, 1, 1459, 16};
        mss[f] = ms[f % 5];
        const uint32_t nseg = f % 7 == 3 ? 0 : mss[f] == 1 ? 70 : 1 + (uint32_t)(next_u64() % 44);
        pay_len[f] = nseg ? nseg * mss[f] - (uint32_t)(next_u64() % mss[f]) : 0;
        hl8[f] = (uint8_t)make_template(tmpl + f * STRIDE, (int)(f % 4), 0xFFFFFF00u + f, (uint16_t)(0xFFF0 + f));
        at = ((at + 15) & ~15ull) + f % 16;  /* every byte alignment */
        pay_off[f] = at;
        at += pay_len[f];
    }
    CHECK(at <= PAY_BYTES, "the sends fit the payload region");

    /* the layout helper, called once for the segment total and again for blk_flow */
    uint64_t n_seg64 = 0, head_end = 0;
    const uint64_t head_first = PAY_BYTES + 1;  /* heads from an odd offset */
    CHECK(rns_tx_segment_layout(pay_len, mss, hl8, NFL, head_first, seg_first, head_off, NULL, NULL, &head_end) ==
              RNS_E_INVALID, "NULL n_seg");
    CHECK(rns_tx_segment_layout(pay_len, mss, hl8, NFL, head_first, seg_first, head_off, NULL, &n_seg64, &head_end) == RNS_OK,
          "layout");
    const uint32_t n_seg = (uint32_t)n_seg64, nblk = (n_seg + 63) / 64;
    CHECK(n_seg > 1000 && n_seg <= MAXSEG && head_end <= ARENA, "%u segments, heads end at %llu", n_seg,
          (unsigned long long)head_end);
    CHECK(rns_tx_segment_layout(pay_len, mss, hl8, NFL, head_first, seg_first, head_off, blk_flow, &n_seg64, &head_end) ==
              RNS_OK, "layout with blk_flow");
    uint64_t h = head_first;
    for (uint32_t f = 0; f < NFL; ++f) {
        const uint32_t nseg = (pay_len[f] + mss[f] - 1) / mss[f];
        CHECK(seg_first[f + 1] - seg_first[f] == nseg && head_off[f] == h, "flow %u", f);
        h += (uint64_t)nseg * hl8[f];
    }
    for (uint32_t b = 0; b < nblk; ++b)
        CHECK(seg_first[blk_flow[b]] <= 64 * b && 64 * b < seg_first[blk_flow[b] + 1], "blk_flow[%u]", b);
    CHECK(rns_tx_segment_chains(pay_off, pay_len, mss, hl8, head_off, NFL, n_seg - 1, frag_off, frag_len, first) ==
              RNS_E_INVALID, "a wrong segment total");
    CHECK(rns_tx_segment_chains(pay_off, pay_len, mss, hl8, head_off, NFL, n_seg, frag_off, frag_len, first) == RNS_OK,
          "chains");

    /* argument checks need no device */
    CHECK(rns_tx_segment_dev(NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == RNS_OK, "empty");
    CHECK(rns_tx_segment_dev(arena, ARENA, tmpl, 0, hl8, pay_off, pay_len, mss, head_off, seg_first, blk_flow, NFL, n_seg,
                             status, NULL) == RNS_E_INVALID, "tmpl_stride 0");
    CHECK(rns_tx_segment_dev(arena, ARENA, NULL, STRIDE, hl8, pay_off, pay_len, mss, head_off, seg_first, blk_flow, NFL, n_seg,
                             status, NULL) == RNS_E_INVALID, "NULL templates");
    CHECK(rns_tx_segment_dev(arena, ARENA, tmpl, STRIDE, hl8, pay_off, pay_len, mss, head_off, seg_first, NULL, NFL, n_seg,
                             status, NULL) == RNS_E_INVALID, "NULL blk_flow");

    uint8_t *d_arena = NULL, *d_tmpl = NULL, *d_hl = NULL, *d_status = NULL;
    uint16_t *d_mss = NULL;
    uint32_t *d_pl = NULL, *d_sf = NULL, *d_bf = NULL;
    uint64_t *d_po = NULL, *d_ho = NULL;
    hipStream_t st;
    UP(d_hl, hl8, NFL);
    UP(d_mss, mss, sizeof mss);
    UP(d_pl, pay_len, sizeof pay_len);
    UP(d_sf, seg_first, sizeof seg_first);
    UP(d_bf, blk_flow, sizeof blk_flow);
    UP(d_po, pay_off, sizeof pay_off);
    UP(d_ho, head_off, sizeof head_off);
    HIP_OK(abi_stream(&st));
    for (int round = 0; round < 2; ++round) {
        if (round == 1)  /* one template with a bad version: that send alone is rejected, its head range untouched */
            tmpl[BAD_FLOW * STRIDE] = 0x75;
        /* the expected arena: the heads built here, finalized by the oracle over the good sends' chains */
        memcpy(want, arena, ARENA);
        uint32_t nch = 0;
        memset(want_st, RNS_TX_MALFORMED, sizeof want_st);
        static uint64_t c_off[2 * MAXSEG];
        static uint32_t c_len[2 * MAXSEG], c_first[MAXSEG + 1], c_seg[MAXSEG];
        static uint8_t c_st[MAXSEG];
        for (uint32_t f = 0; f < NFL; ++f) {
            if (round == 1 && f == BAD_FLOW)
                continue;
            for (uint32_t s = seg_first[f]; s < seg_first[f + 1]; ++s, ++nch) {
                const uint32_t j = s - seg_first[f];
                CHECK(first[s] == 2 * s && frag_off[2 * s] == head_off[f] + (uint64_t)j * hl8[f] && frag_len[2 * s] == hl8[f] &&
                          frag_off[2 * s + 1] == pay_off[f] + (uint64_t)j * mss[f], "chain of segment %u", s);
                make_segment_head(want + frag_off[2 * s], tmpl + f * STRIDE, hl8[f], j, mss[f], frag_len[2 * s + 1]);
                c_first[nch] = 2 * nch;
                c_off[2 * nch] = frag_off[2 * s]; c_len[2 * nch] = frag_len[2 * s];
                c_off[2 * nch + 1] = frag_off[2 * s + 1]; c_len[2 * nch + 1] = frag_len[2 * s + 1];
                c_seg[nch] = s;
            }
        }
        c_first[nch] = 2 * nch;
        oracle_tx_chain_fill(want, ARENA, c_off, c_len, c_first, 2 * nch, nch, c_st);
        for (uint32_t k = 0; k < nch; ++k) {
            want_st[c_seg[k]] = c_st[k];
            CHECK(c_st[k] == RNS_TX_L4_FILLED || c_st[k] == (RNS_TX_IP_FILLED | RNS_TX_L4_FILLED), "the oracle: chain %u", k);
        }
        CHECK(round == 0 ? nch == n_seg : nch < n_seg, "round %d: %u chains", round, nch);

        UP(d_arena, arena, ARENA);
        UP(d_tmpl, tmpl, sizeof tmpl);
        OUT(d_status, MAXSEG, 0x55);
        CHECK(rns_tx_segment_dev(d_arena, ARENA, d_tmpl, STRIDE, d_hl, d_po, d_pl, d_mss, d_ho, d_sf, d_bf, NFL, n_seg, d_status,
                                 st) == RNS_OK, "rns_tx_segment_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(status, d_status, MAXSEG);
        DOWN(back, d_arena, ARENA);
        for (uint32_t i = 0; i < n_seg; ++i)
            CHECK(status[i] == want_st[i], "round %d status %u: %02x != %02x", round, i, status[i], want_st[i]);
        for (uint32_t i = n_seg; i < MAXSEG; ++i)
            CHECK(status[i] == 0x55, "round %d status %u past n_seg written", round, i);
        for (size_t b = 0; b < ARENA; ++b)
            CHECK(back[b] == want[b], "round %d arena byte %zu: %02x != %02x", round, b, back[b], want[b]);
    }
    /* without the status array: the same bytes */
    UP(d_arena, arena, ARENA);
    CHECK(rns_tx_segment_dev(d_arena, ARENA, d_tmpl, STRIDE, d_hl, d_po, d_pl, d_mss, d_ho, d_sf, d_bf, NFL, n_seg, NULL, st) ==
              RNS_OK, "no status array");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(back, d_arena, ARENA);
    CHECK(memcmp(back, want, ARENA) == 0, "without the status array: the arena differs");
    return abi_finish("%u segments of %d sends", n_seg, NFL);
}
