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
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rns_checksum.h"

int32_t oracle_compute_ones_comp(uint16_t in_checksum, const uint8_t *slice, size_t len);
int32_t oracle_compute_checksum(const uint8_t *slice, size_t len);
int32_t oracle_compute_buffer_ones_comp(uint16_t initial_sum, const uint8_t *const *frag_base, const size_t *frag_len,
                                        size_t nfrags);
int32_t oracle_compute_pseudo_header_checksum(const uint8_t *src, size_t src_len, const uint8_t *dst, size_t dst_len,
                                              uint64_t length, uint8_t protocol);

static uint64_t rng_state = 0x71ACE5EEDull;
static uint64_t next_u64(void)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (failures++ < 10) {                                                                 \
                fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                               \
                fprintf(stderr, __VA_ARGS__);                                                      \
                fprintf(stderr, "\n");                                                             \
            }                                                                                      \
        }                                                                                          \
    } while (0)
#define HIP_OK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));              \
            return 2;                                                                              \
        }                                                                                          \
    } while (0)

enum { N = 200, NFLOW = 3, LOG2 = 9, BUF = 1 << LOG2, MAXLEN = 1600, MAXFR = (MAXLEN + BUF - 1) / BUF, NBUF = N * MAXFR,
       NBLK = (N + 63) / 64, WIN = 1 << 17, STREAM = NFLOW * WIN + 64, SENTINEL = 0xA7 };

static const uint8_t local4[4] = {10, 0, 0, 2}, remote4[4] = {10, 0, 0, 1}, other4[4] = {10, 0, 9, 9};
static uint8_t local6[16], remote6[16];

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
    seg[0] = (uint8_t)(sport >> 8); seg[1] = (uint8_t)sport; seg[2] = (uint8_t)(f->dport >> 8); seg[3] = (uint8_t)f->dport;
    seg[4] = (uint8_t)(seq >> 24); seg[5] = (uint8_t)(seq >> 16); seg[6] = (uint8_t)(seq >> 8); seg[7] = (uint8_t)seq;
    seg[8] = 0xA1; seg[9] = 0xB2; seg[10] = 0xC3; seg[11] = 0xD4;
    seg[12] = (uint8_t)((f->tcp_hdr / 4) << 4); seg[13] = 0x18; seg[14] = 0x12; seg[15] = 0x34;
    memcpy(seg + f->tcp_hdr, pay, n);
    if (f->v6) {
        p[0] = 0x60; p[4] = (uint8_t)(sl >> 8); p[5] = (uint8_t)sl; p[6] = 6; p[7] = 64;
        memcpy(p + 8, f->src, 16);
        memcpy(p + 24, local6, 16);
    } else {
        p[0] = (uint8_t)(0x40 | (f->ip_hdr / 4)); p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)len; p[8] = 64; p[9] = 6;
        memcpy(p + 12, f->src, 4);
        memcpy(p + 16, local4, 4);
        const uint16_t c = (uint16_t)oracle_compute_checksum(p, f->ip_hdr);
        p[10] = (uint8_t)(c >> 8); p[11] = (uint8_t)c;
    }
    const uint16_t ph = (uint16_t)oracle_compute_pseudo_header_checksum(f->src, f->v6 ? 16 : 4, f->v6 ? local6 : local4,
                                                                        f->v6 ? 16 : 4, sl, 6);
    const uint16_t c = (uint16_t)(0xffff ^ oracle_compute_ones_comp(ph, seg, sl));
    seg[16] = (uint8_t)(c >> 8); seg[17] = (uint8_t)c;
    return len;
}

static uint32_t make_icmp(uint8_t *p, uint32_t n)
{
    const uint32_t len = 20 + 8 + n;
    memset(p, 0, 28);
    for (uint32_t b = 28; b < len; ++b)
        p[b] = (uint8_t)next_u64();
    p[0] = 0x45; p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)len; p[8] = 64; p[9] = 1;
    memcpy(p + 12, remote4, 4);
    memcpy(p + 16, local4, 4);
    uint16_t c = (uint16_t)oracle_compute_checksum(p, 20);
    p[10] = (uint8_t)(c >> 8); p[11] = (uint8_t)c;
    p[20] = 8;
    c = (uint16_t)(0xffff ^ oracle_compute_ones_comp(0, p + 20, len - 20));
    p[22] = (uint8_t)(c >> 8); p[23] = (uint8_t)c;
    return len;
}

/* The receive path over a datagram of `total` bytes in the buffers idx[0..): the header from the
 * first buffer, trim_head, compute_buffer_ones_comp over the trimmed fragments. */
static void reference(const uint8_t *pool, const uint32_t *idx, uint32_t total, uint8_t *status, uint16_t *l4)
{
    const uint8_t *header = pool + (uint64_t)idx[0] * BUF;
    const int v6 = (header[0] >> 4) == 6;
    const uint32_t hdr = v6 ? 40 : (header[0] & 0xfu) * 4u;
    uint8_t st = (v6 || oracle_compute_checksum(header, hdr) == 0) ? RNS_RX_IP_OK : 0;
    const uint8_t proto = v6 ? header[6] : header[9];
    const uint8_t *base[MAXFR];
    size_t len[MAXFR];
    size_t k = 0;
    for (uint32_t f = 0, pos = 0; pos < total; ++f, pos += BUF) {
        const uint32_t fl = total - pos < BUF ? total - pos : BUF, cut = f == 0 ? hdr : 0;
        if (fl > cut) {
            base[k] = pool + (uint64_t)idx[f] * BUF + cut;
            len[k++] = fl - cut;
        }
    }
    const uint16_t ph = proto == 1 ? 0
        : (uint16_t)oracle_compute_pseudo_header_checksum(header + (v6 ? 8 : 12), v6 ? 16 : 4, v6 ? local6 : local4,
                                                          v6 ? 16 : 4, total - hdr, proto);
    *l4 = (uint16_t)(0xffff ^ (k ? oracle_compute_buffer_ones_comp(ph, base, len, k) : ph));
    if (*l4 == 0)
        st |= RNS_RX_L4_OK;
    if ((st & RNS_RX_IP_OK) && (st & RNS_RX_L4_OK))
        st |= RNS_RX_ACCEPT;
    *status = st;
}

int main(void)
{
    for (int b = 0; b < 16; ++b) {
        local6[b] = (uint8_t)(b == 0 ? 0xfd : b == 15 ? 2 : 0);
        remote6[b] = (uint8_t)(b == 0 ? 0xfd : b == 15 ? 1 : 0);
    }
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
        for (uint32_t b = 0; b < WIN; ++b)
            data[f][b] = (uint8_t)next_u64();
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
    for (uint32_t j = 0; j < N; ++j)
        order[j] = j;
    for (uint32_t j = N - 1; j > 0; --j) {
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j];
        order[j] = order[r];
        order[r] = t;
    }
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
    for (uint32_t j = 0; j < NBUF; ++j)
        order[j] = j;
    for (uint32_t j = NBUF - 1; j > 0; --j) {
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j];
        order[j] = order[r];
        order[r] = t;
    }
    memset(pool, 0xEE, sizeof pool);
    int placed = 0, unmatched = 0, undecoded = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t dl = len16[i];
        for (uint32_t f = first[i], pos = 0; f < first[i + 1]; ++f, pos += BUF) {
            idx[f] = order[f];
            memcpy(pool + ((uint64_t)idx[f] << LOG2), dgrams[i] + pos, dl - pos < BUF ? dl - pos : BUF);
        }
        reference(pool, idx + first[i], dl, &ref_status[i], &ref_l4[i]);
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
        m->sport = (uint16_t)(h[0] << 8 | h[1]);
        m->dport = (uint16_t)(h[2] << 8 | h[3]);
        m->seq = (uint32_t)h[4] << 24 | (uint32_t)h[5] << 16 | (uint32_t)h[6] << 8 | h[7];
        m->ack = (uint32_t)h[8] << 24 | (uint32_t)h[9] << 16 | (uint32_t)h[10] << 8 | h[11];
        m->flags = h[13];
        m->window = (uint16_t)(h[14] << 8 | h[15]);
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
    if (hipMalloc((void **)&d_pool, sizeof pool) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed: no usable device\n");
        return 2;
    }
    HIP_OK(hipMalloc((void **)&d_status, N));
    HIP_OK(hipMalloc((void **)&d_l4, N * sizeof *l4));
    HIP_OK(hipMalloc((void **)&d_len16, N * sizeof *len16));
    HIP_OK(hipMalloc((void **)&d_idx, NBUF * sizeof *idx));
    HIP_OK(hipMalloc((void **)&d_blk, NBLK * sizeof *blk_first));
    HIP_OK(hipMalloc((void **)&d_tbl, need));
    HIP_OK(hipMalloc((void **)&d_next, sizeof next_seq));
    HIP_OK(hipMalloc((void **)&d_woff, sizeof win_off));
    HIP_OK(hipMalloc((void **)&d_wlen, sizeof win_len));
    HIP_OK(hipMalloc((void **)&d_stream, STREAM));
    HIP_OK(hipMalloc((void **)&d_meta, sizeof meta));
    HIP_OK(hipStreamCreate(&st));
    HIP_OK(hipMemcpy(d_pool, pool, sizeof pool, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_len16, len16, N * sizeof *len16, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_idx, idx, NBUF * sizeof *idx, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_blk, blk_first, NBLK * sizeof *blk_first, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tbl, table, need, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_next, next_seq, sizeof next_seq, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_woff, win_off, sizeof win_off, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_wlen, win_len, sizeof win_len, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_stream, SENTINEL, STREAM));
    HIP_OK(hipMemset(d_status, 0x55, N));
    HIP_OK(hipMemset(d_meta, 0xEE, sizeof meta));
    CHECK(rns_rx_tcp_place_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_tbl, need,
                                    d_next, d_woff, d_wlen, NFLOW, d_stream, STREAM, d_status, d_l4, d_meta, st) == RNS_OK,
          "rns_rx_tcp_place_pool_dev");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(l4, d_l4, N * sizeof *l4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(meta, d_meta, sizeof meta, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(stream, d_stream, STREAM, hipMemcpyDeviceToHost));
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
    HIP_OK(hipMemcpy(back, d_pool, sizeof pool, hipMemcpyDeviceToHost));
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    hipStreamDestroy(st);
    hipFree(d_pool); hipFree(d_status); hipFree(d_l4); hipFree(d_len16); hipFree(d_idx); hipFree(d_blk); hipFree(d_tbl);
    hipFree(d_next); hipFree(d_woff); hipFree(d_wlen); hipFree(d_stream); hipFree(d_meta);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
