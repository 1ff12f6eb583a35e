/*
 * A plain C caller of TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev) and the
 * flow table's host helper (rns_rx_flow_table_build), bound the way the reference's Rust would bind
 * them (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for device memory.
 * 200 datagrams — the segments of three flows (IPv4, IPv6, IPv4 with IP and TCP options) in a
 * shuffled order, every seventh with a flipped byte, every eleventh from a port no flow has, some
 * ICMP between them — lie in shuffled 512-byte pool buffers as recv_packet leaves them
 * (netif.rs:65-83).  Every status and L4 value is checked against the receive path restated here
 * over the oracle's primitives (oracle/csum_oracle.c, linked as test infrastructure only), every
 * meta record and every byte of the stream arena against values computed here.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x71ACE5EEDull
#include "abi_test.h"

enum { N = 200, NFLOW = 3, LOG2 = 9, BUF = 1 << LOG2, MAXLEN = 1600, MAXFR = (MAXLEN + BUF - 1) / BUF, NBUF = N * MAXFR,
       NBLK = (N + 63) / 64, WIN = 1 << 17, STREAM = NFLOW * WIN + 64, SENTINEL = 0xA7 };

static const uint8_t local4[4] = {10, 0, 0, 2}, remote4[4] = {10, 0, 0, 1}, other4[4] = {10, 0, 9, 9};
static const uint8_t local6[16] = {0xfd, [15] = 2}, remote6[16] = {0xfd, [15] = 1};

typedef struct flow {
    int v6;
    const uint8_t *src;
    uint16_t sport, dport;
    uint32_t ip_hdr, tcp_hdr, next_seq;
} flow;

/* A valid TCP datagram of flow f with the given sequence number and payload in p; returns its length. */
static uint32_t make_segment(uint8_t *p, const flow *f, uint16_t sport, uint32_t seq, const uint8_t *pay, uint32_t n)
{
    const uint32_t len = f->ip_hdr + f->tcp_hdr + n, sl = f->tcp_hdr + n;
    memset(p, 1, f->ip_hdr + f->tcp_hdr);  /* options: NOPs */
    memset(p, 0, f->v6 ? 40 : 20);
    uint8_t *seg = p + f->ip_hdr;
    memset(seg, 0, 20);
    put16(seg, sport); put16(seg + 2, f->dport); put32(seg + 4, seq); put32(seg + 8, 0xA1B2C3D4u);
    seg[12] = (uint8_t)((f->tcp_hdr / 4) << 4); seg[13] = 0x18; put16(seg + 14, 0x1234);
    memcpy(seg + f->tcp_hdr, pay, n);
    if (f->v6) {
        ipv6_header(p, sl, 6, f->src, local6);
    } else {
        p[0] = (uint8_t)(0x40 | (f->ip_hdr / 4)); p[8] = 64; p[9] = 6;
        ipv4_finish(p, f->ip_hdr, len, f->src, local4);
    }
    l4_checksum(seg, sl, 16, f->src, f->v6 ? local6 : local4, f->v6 ? 16 : 4, 6);
    return len;
}

static uint32_t make_icmp(uint8_t *p, uint32_t n)
{
    const uint32_t len = 20 + 8 + n;
    memset(p, 0, 28);
    fill_random_bytes(p + 28, len - 28);
    p[0] = 0x45; p[8] = 64; p[9] = 1;
    ipv4_finish(p, 20, len, remote4, local4);
    p[20] = 8;
    l4_checksum(p + 20, len - 20, 2, NULL, NULL, 0, 1);
    return len;
}

int main(void)
{
    const flow flows[NFLOW] = {{0, remote4, 40000, 80, 20, 20, 0xFFFFF000u},
                               {1, remote6, 40001, 443, 40, 32, 1000u},
                               {0, other4, 40000, 80, 24, 28, 0x80000000u}};
    static uint8_t pool[NBUF * BUF], dgrams[N][MAXLEN], data[NFLOW][WIN], status[N], ref_status[N], stream[STREAM],
        ref_stream[STREAM];
    static uint16_t len16[N], l4[N], ref_l4[N];
    static uint32_t idx[NBUF], blk_first[NBLK], first[N + 1], order[NBUF], win_len[NFLOW], next_seq[NFLOW];
    static uint64_t win_off[NFLOW];
    static rns_rx_tcp_meta meta[N], ref_meta[N];
    static rns_rx_flow_key keys[NFLOW];

    /* the flows' keys, their table, their windows */
    memset(keys, 0, sizeof keys);
    for (int f = 0; f < NFLOW; ++f) {
        memcpy(keys[f].ip, flows[f].src, flows[f].v6 ? 16 : 4);
        keys[f].sport = flows[f].sport;
        keys[f].dport = flows[f].dport;
        keys[f].family = flows[f].v6 ? 6 : 4;
        win_off[f] = 32 + (uint64_t)f * WIN + (uint64_t)f * 5;  /* every destination alignment in turn */
        win_len[f] = WIN - 16;
        next_seq[f] = flows[f].next_seq;
        fill_random_bytes(data[f], WIN);
    }
    uint64_t need = 0;
    static uint8_t table[64 * 32 + 8];
    memset(table, 0xC3, sizeof table);
    CHECK(rns_rx_flow_table_build(keys, NFLOW, NULL, 0, &need) == RNS_OK && need == 64 * 32, "size query: %llu",
          (unsigned long long)need);
    CHECK(rns_rx_flow_table_build(keys, NFLOW, table, need, NULL) == RNS_E_INVALID, "NULL need_bytes");
    CHECK(rns_rx_flow_table_build(keys, NFLOW, table, need - 1, &need) == RNS_E_INVALID, "a short table");
    CHECK(rns_rx_flow_table_build(keys, NFLOW, table, need, &need) == RNS_OK, "rns_rx_flow_table_build");
    CHECK(table[need] == 0xC3 && table[need + 7] == 0xC3, "written past the table");

    /* the datagrams: each flow's stream cut into segments, in a shuffled order */
    memset(ref_stream, SENTINEL, sizeof ref_stream);
    uint32_t sent[NFLOW] = {0, 0, 0};
    for (uint32_t i = 0; i < N; ++i) {
        if (i % 13 == 12) {
            len16[i] = (uint16_t)make_icmp(dgrams[i], (uint32_t)(next_u64() % 900));
            continue;
        }
        const int f = (int)(i % NFLOW);
        const uint32_t hdr = flows[f].ip_hdr + flows[f].tcp_hdr;
        const uint32_t edge[] = {0, 1, 15, 16, 17, BUF - hdr, BUF - hdr + 1, MAXLEN - hdr};
        const uint32_t n = i < 24 ? edge[i / 3] : (uint32_t)(next_u64() % (MAXLEN - hdr + 1));
        const uint16_t sport = (uint16_t)(flows[f].sport + (i % 11 == 10 ? 7 : 0));  /* a port no flow has */
        len16[i] = (uint16_t)make_segment(dgrams[i], &flows[f], sport, flows[f].next_seq + sent[f], data[f] + sent[f], n);
        sent[f] += n;
        CHECK(sent[f] <= win_len[f], "flow %d sends %u bytes", f, sent[f]);
    }
    shuffled_order(order, N);
    static uint8_t tmp[N][MAXLEN];
    static uint16_t tlen[N];
    memcpy(tmp, dgrams, sizeof tmp);
    memcpy(tlen, len16, sizeof tlen);
    for (uint32_t j = 0; j < N; ++j) {
        memcpy(dgrams[j], tmp[order[j]], MAXLEN);
        len16[j] = tlen[order[j]];
        if (j % 7 == 6)
            dgrams[j][len16[j] - 1 - next_u64() % 8] ^= 0x20;  /* a flipped byte near the end */
    }

    /* into shuffled pool buffers */
    uint64_t nf64 = 0;
    CHECK(rns_rx_pool_layout(len16, N, LOG2, blk_first, first, &nf64) == RNS_OK, "layout");
    const uint32_t nf = (uint32_t)nf64;
    shuffled_order(order, NBUF);
    memset(pool, 0xEE, sizeof pool);
    int placed = 0, unmatched = 0, undecoded = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t dl = len16[i];
        for (uint32_t f = first[i], pos = 0; f < first[i + 1]; ++f, pos += BUF) {
            idx[f] = order[f];
            memcpy(pool + ((uint64_t)idx[f] << LOG2), dgrams[i] + pos, dl - pos < BUF ? dl - pos : BUF);
        }
        rx_reference_pool(pool, LOG2, idx + first[i], dl, local4, local6, &ref_status[i], &ref_l4[i]);
        /* tcp.rs:549-574, the lookup and the placement rule, over the flat datagram */
        const uint8_t *p = dgrams[i];
        rns_rx_tcp_meta *m = &ref_meta[i];
        memset(m, 0, sizeof *m);
        m->flow = RNS_RX_NO_FLOW;
        const int v6 = (p[0] >> 4) == 6;
        const uint32_t ip_hdr = v6 ? 40 : (p[0] & 0xfu) * 4u;
        if (!(ref_status[i] & RNS_RX_ACCEPT) || (v6 ? p[6] : p[9]) != 6 || dl - ip_hdr < 20) {
            ++undecoded;
            continue;
        }
        const uint8_t *h = p + ip_hdr;
        const uint32_t tcp_hdr = (uint32_t)(h[12] >> 4) * 4;
        CHECK(tcp_hdr >= 20 && tcp_hdr <= dl - ip_hdr, "datagram %u: data offset", i);
        m->sport = (uint16_t)get16(h);
        m->dport = (uint16_t)get16(h + 2);
        m->seq = get32(h + 4);
        m->ack = get32(h + 8);
        m->flags = h[13];
        m->window = (uint16_t)get16(h + 14);
        m->pay_len = (uint16_t)(dl - ip_hdr - tcp_hdr);
        m->ip_hdr = (uint8_t)ip_hdr;
        m->tcp_hdr = (uint8_t)tcp_hdr;
        m->place = RNS_PLACE_TCP;
        for (int f = 0; f < NFLOW; ++f)
            if (flows[f].v6 == v6 && memcmp(p + (v6 ? 8 : 12), flows[f].src, v6 ? 16 : 4) == 0 &&
                flows[f].sport == m->sport && flows[f].dport == m->dport)
                m->flow = (uint32_t)f;
        if (m->flow == RNS_RX_NO_FLOW) {
            ++unmatched;
            continue;
        }
        m->place |= RNS_PLACE_FLOW;
        if (m->pay_len == 0)
            continue;
        const uint32_t d = m->seq - next_seq[m->flow];
        CHECK(d < win_len[m->flow] && m->pay_len <= win_len[m->flow] - d, "datagram %u lies in its window", i);
        m->place |= RNS_PLACE_DONE;
        memcpy(ref_stream + win_off[m->flow] + d, h + tcp_hdr, m->pay_len);
        ++placed;
    }
    CHECK(placed > 100 && unmatched > 5 && undecoded > 30, "placed %d, unmatched %d, undecoded %d", placed, unmatched,
          undecoded);

    /* argument checks need no device */
    CHECK(rns_rx_tcp_place_pool_dev(NULL, 0, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, 0,
                                    NULL, NULL, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_rx_tcp_place_pool_dev(pool, sizeof pool, LOG2, idx, nf, blk_first, len16, N, local4, local6, table, need,
                                    next_seq, win_off, win_len, NFLOW, stream, STREAM, status, NULL, NULL, NULL) ==
              RNS_E_INVALID, "NULL meta");
    CHECK(rns_rx_tcp_place_pool_dev(pool, sizeof pool, 6, idx, nf, blk_first, len16, N, local4, local6, table, need,
                                    next_seq, win_off, win_len, NFLOW, stream, STREAM, status, NULL, meta, NULL) ==
              RNS_E_INVALID, "buf_log2 6");
    CHECK(rns_rx_tcp_place_pool_dev(pool, sizeof pool, LOG2, idx, nf, blk_first, len16, N, local4, local6, NULL, need,
                                    next_seq, win_off, win_len, NFLOW, stream, STREAM, status, NULL, meta, NULL) ==
              RNS_E_INVALID, "NULL table");

    uint8_t *d_pool = NULL, *d_status = NULL, *d_tbl = NULL, *d_stream = NULL;
    uint16_t *d_l4 = NULL, *d_len16 = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL, *d_next = NULL, *d_wlen = NULL;
    uint64_t *d_woff = NULL;
    rns_rx_tcp_meta *d_meta = NULL;
    hipStream_t st;
    UP(d_pool, pool, sizeof pool);
    UP(d_len16, len16, N * sizeof *len16);
    UP(d_idx, idx, NBUF * sizeof *idx);
    UP(d_blk, blk_first, NBLK * sizeof *blk_first);
    UP(d_tbl, table, need);
    UP(d_next, next_seq, sizeof next_seq);
    UP(d_woff, win_off, sizeof win_off);
    UP(d_wlen, win_len, sizeof win_len);
    OUT(d_stream, STREAM, SENTINEL);
    OUT(d_status, N, 0x55);
    OUT(d_l4, N * sizeof *l4, 0);
    OUT(d_meta, sizeof meta, 0xEE);
    HIP_OK(abi_stream(&st));
    CHECK(rns_rx_tcp_place_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_tbl, need,
                                    d_next, d_woff, d_wlen, NFLOW, d_stream, STREAM, d_status, d_l4, d_meta, st) == RNS_OK,
          "rns_rx_tcp_place_pool_dev");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(status, d_status, N);
    DOWN(l4, d_l4, N * sizeof *l4);
    DOWN(meta, d_meta, sizeof meta);
    DOWN(stream, d_stream, STREAM);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
        CHECK(l4[i] == ref_l4[i], "l4 %u: %04x != %04x", i, l4[i], ref_l4[i]);
        const rns_rx_tcp_meta *g = &meta[i], *w = &ref_meta[i];
        CHECK(g->flow == w->flow && g->seq == w->seq && g->ack == w->ack && g->sport == w->sport && g->dport == w->dport &&
                  g->window == w->window && g->pay_len == w->pay_len && g->flags == w->flags && g->ip_hdr == w->ip_hdr &&
                  g->tcp_hdr == w->tcp_hdr && g->place == w->place,
              "meta %u: flow %x/%x seq %x/%x pay_len %u/%u place %x/%x", i, g->flow, w->flow, g->seq, w->seq, g->pay_len,
              w->pay_len, g->place, w->place);
    }
    for (uint32_t b = 0; b < STREAM; ++b)
        CHECK(stream[b] == ref_stream[b], "stream byte %u: %02x != %02x", b, stream[b], ref_stream[b]);
    static uint8_t back[sizeof pool];
    DOWN(back, d_pool, sizeof pool);
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    return abi_finish("%d datagrams: %d placed, %d of no flow, %d not decoded", N, placed, unmatched, undecoded);
}
