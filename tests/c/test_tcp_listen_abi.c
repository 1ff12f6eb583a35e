/*
 * A plain C caller of the TCP listen responder (rns_rx_tcp_listen_pool_dev, rns_rx_tcp_listen_work), bound the way
 * the reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for
 * device memory.  600 datagrams in a shuffled pool of 128-byte buffers with the records the placement would leave
 * for them: SYNs and other segments from 40 IPv4 and IPv6 peers to three ports, two of them listening (so keys
 * repeat: strays before a SYN, duplicate SYNs, segments after it), segments of known flows, and datagrams that are
 * no TCP.  The program walks the batch the way tcp_input does (tcp.rs:576-615: a PORT_MAP that grows with every
 * new connection) and builds every reply itself the way tcp_output and ip_output do (tcp.rs:938-976,
 * ip.rs:140-177), then compares d_conn, every slot, the descriptors, the accept records and d_count, and that
 * nothing else is written; then once more with a reply cap, and with no slots at all.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x7C9115EEull
#include "abi_test.h"

enum { N = 600, LOG2 = 7, BUF = 1 << LOG2, NBUF = N + 5, PEERS = 40, FILL = 0x55 };

static const uint8_t L4[4] = {10, 0, 0, 2}, R4[4] = {10, 0, 0, 1};
static const uint8_t L6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
static const uint8_t R6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
static const uint16_t PORTS[3] = {80, 443, 8080};  /* 8080: nobody listens */

static uint8_t pool[NBUF * BUF], out[N * 64], rep_len8[N], conn[N], want[64];
static uint16_t len16[N], listen_tbl[65536];
static uint32_t buf_idx[NBUF], blk_first[(N + 63) / 64], rep_src[N], iss[N], count[3];
static rns_rx_tcp_meta meta[N];
static rns_tcp_accept accept[N];
static int opened[PEERS][3];  /* PORT_MAP's growth: the key (peer, its port, the local port) has a socket */

/* tcp_output -> ip_output for an empty segment from the local address to peer p's address: its length, in `want`. */
static uint32_t build(int v6, const uint8_t *remote, uint32_t sport, uint32_t dport, uint32_t seq, uint32_t ack, int syn, uint32_t id)
{
    const uint32_t h = v6 ? 40 : 20, tl = syn ? 24 : 20;
    memset(want, 0, sizeof want);
    uint8_t *t = want + h;
    put16(t, sport);
    put16(t + 2, dport);
    put32(t + 4, seq);
    put32(t + 8, ack);
    t[12] = (uint8_t)((tl / 4) << 4);
    t[13] = syn ? 0x12 : 0x14;
    put16(t + 14, syn ? 0xffff : 0);
    if (syn) { t[20] = 2; t[21] = 4; t[22] = 0x05; t[23] = 0xdc; }
    l4_checksum(t, tl, 16, v6 ? L6 : L4, remote, v6 ? 16 : 4, 6);
    if (v6) {
        ipv6_header(want, tl, 6, L6, remote);
    } else {
        want[0] = 0x45; put16(want + 2, 20 + tl); put16(want + 4, id); want[8] = 64; want[9] = 6;
        memcpy(want + 12, L4, 4);
        memcpy(want + 16, remote, 4);
        ipv4_checksum(want, 20);
    }
    return h + tl;
}

int main(void)
{
    /* the batch: datagram i from peer i's draw; kind 0..5: SYN, SYN with MSS, ACK, RST, a known flow's, no TCP */
    static int peer[N], port[N], kind[N];
    static uint8_t remote[N][16];
    shuffled_order(buf_idx, NBUF);
    fill_random_bytes(pool, sizeof pool);
    for (int p = 0; p < 65536; ++p)
        listen_tbl[p] = RNS_UDP_NO_SOCK;
    listen_tbl[80] = 0;
    listen_tbl[443] = 1;
    listen_tbl[8080] = 7;  /* an entry >= n_listen is no listener */
    for (uint32_t i = 0; i < N; ++i) {
        peer[i] = (int)(next_u64() % PEERS);
        port[i] = (int)(next_u64() % 3);
        kind[i] = (int)(next_u64() % 6);
        const int v6 = peer[i] & 1;
        const uint32_t h = v6 ? 40 : 20, th = kind[i] == 1 ? 24 : 20, pay = kind[i] == 2 ? (uint32_t)(next_u64() % 40) : 0;
        uint8_t *d = pool + ((size_t)buf_idx[i] << LOG2);
        memcpy(remote[i], v6 ? R6 : R4, v6 ? 16 : 4);
        remote[i][v6 ? 15 : 3] = (uint8_t)(1 + peer[i]);
        len16[i] = (uint16_t)(h + th + pay);
        memset(d, 0, h + th);
        if (v6) {
            ipv6_header(d, th + pay, 6, remote[i], L6);
        } else {
            d[0] = 0x45; d[8] = 64; d[9] = 6;
            ipv4_finish(d, 20, h + th + pay, remote[i], L4);
        }
        memset(&meta[i], 0, sizeof meta[i]);
        meta[i].flow = kind[i] == 4 ? (uint32_t)peer[i] : RNS_RX_NO_FLOW;
        meta[i].seq = (uint32_t)next_u64();
        meta[i].ack = (uint32_t)next_u64();
        meta[i].sport = (uint16_t)(30000 + peer[i]);
        meta[i].dport = PORTS[port[i]];
        meta[i].window = (uint16_t)next_u64();
        meta[i].pay_len = (uint16_t)pay;
        meta[i].flags = kind[i] <= 1 ? 0x02 : kind[i] == 3 ? 0x04 : 0x10;
        meta[i].ip_hdr = (uint8_t)h;
        meta[i].tcp_hdr = (uint8_t)th;
        meta[i].place = kind[i] == 5 ? 0 : kind[i] == 4 ? RNS_PLACE_TCP | RNS_PLACE_FLOW : RNS_PLACE_TCP;
        if (kind[i] == 1) { d[h + 20] = 2; d[h + 21] = 4; d[h + 22] = 0x05; d[h + 23] = 0xb4; }
        iss[i] = (uint32_t)next_u64();
    }
    for (uint32_t b = 0; b < (N + 63) / 64; ++b)
        blk_first[b] = 64 * b;  /* one buffer per datagram */

    /* the workspace size and every argument check need no device */
    uint64_t need = 0, need0 = 0;
    CHECK(rns_rx_tcp_listen_work(N, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_tcp_listen_work(RNS_CHAIN_MAX_PACKETS + 1, &need) == RNS_E_INVALID, "too many datagrams for the workspace");
    CHECK(rns_rx_tcp_listen_work(0, &need0) == RNS_OK && need0 > 0, "work(0)");
    CHECK(rns_rx_tcp_listen_work(N, &need) == RNS_OK && need >= need0, "work(N)");
    uint8_t *fake = (uint8_t *)4096;
    uint32_t *const f32 = (uint32_t *)fake;
    uint16_t *const f16 = (uint16_t *)fake;
    rns_rx_tcp_meta *const fm = (rns_rx_tcp_meta *)fake;
    rns_tcp_accept *const fa = (rns_tcp_accept *)fake;
#define CALL(pl, log2, bi, bf, ln, n, l4, l6, mt, lt, nl, is, o, cap, rs, rl, ac, cnt, cn, wk, wkb) \
    rns_rx_tcp_listen_pool_dev(pl, sizeof pool, log2, bi, NBUF, bf, ln, n, l4, l6, mt, lt, nl, is, 0, NULL, o, cap, rs, rl, ac, cnt, cn, wk, wkb, NULL)
#define BAD(what, ...) CHECK(CALL(__VA_ARGS__) == RNS_E_INVALID, what)
    BAD("NULL pool", NULL, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("misaligned pool", fake + 8, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("buf_log2 6", fake, 6, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("buf_log2 16", fake, 16, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL buf_idx", fake, LOG2, NULL, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL blk_first", fake, LOG2, f32, NULL, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL len16", fake, LOG2, f32, f32, NULL, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("too many datagrams", fake, LOG2, f32, f32, f16, RNS_CHAIN_MAX_PACKETS + 1, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, ~0ull);
    BAD("NULL IPv4 address", fake, LOG2, f32, f32, f16, N, NULL, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL IPv6 address", fake, LOG2, f32, f32, f16, N, L4, NULL, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL meta", fake, LOG2, f32, f32, f16, N, L4, L6, NULL, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("misaligned meta", fake, LOG2, f32, f32, f16, N, L4, L6, (rns_rx_tcp_meta *)(fake + 2), f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL listen table", fake, LOG2, f32, f32, f16, N, L4, L6, fm, NULL, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("too many listeners", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, RNS_UDP_MAX_SOCKS + 1, f32, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL iss", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, NULL, fake, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL out", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, NULL, N, f32, fake, fa, f32, fake, fake, need);
    BAD("misaligned out", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake + 2, N, f32, fake, fa, f32, fake, fake, need);
    BAD("NULL rep_src", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, NULL, fake, fa, f32, fake, fake, need);
    BAD("NULL rep_len8", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, NULL, fa, f32, fake, fake, need);
    BAD("NULL accept", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, NULL, f32, fake, fake, need);
    BAD("misaligned accept", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, (rns_tcp_accept *)(fake + 2), f32, fake, fake, need);
    BAD("NULL counts", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, NULL, fake, fake, need);
    BAD("misaligned counts", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, (uint32_t *)(fake + 2), fake, fake, need);
    BAD("NULL d_conn", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, NULL, fake, need);
    BAD("NULL workspace", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, NULL, need);
    BAD("a misaligned workspace", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake + 4, need);
    BAD("a short workspace", fake, LOG2, f32, f32, f16, N, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, f32, fake, fake, need - 1);
    BAD("no datagrams, NULL counts", fake, LOG2, f32, f32, f16, 0, L4, L6, fm, f16, 2, f32, fake, N, f32, fake, fa, NULL, fake, fake, need);

    uint8_t *d_pool = NULL, *d_out = NULL, *d_rl = NULL, *d_conn = NULL;
    uint16_t *d_len = NULL, *d_tbl = NULL;
    uint32_t *d_idx = NULL, *d_bf = NULL, *d_rs = NULL, *d_iss = NULL, *d_count = NULL, *d_add = NULL;
    rns_rx_tcp_meta *d_meta = NULL;
    rns_tcp_accept *d_acc = NULL;
    void *d_work = NULL;
    hipStream_t st;
    const uint32_t add = 0x2fff0;  /* with the base: the ids wrap */
    UP(d_pool, pool, sizeof pool);
    UP(d_idx, buf_idx, sizeof buf_idx);
    UP(d_bf, blk_first, sizeof blk_first);
    UP(d_len, len16, sizeof len16);
    UP(d_meta, meta, sizeof meta);
    UP(d_tbl, listen_tbl, sizeof listen_tbl);
    UP(d_iss, iss, sizeof iss);
    UP(d_add, &add, sizeof add);
    OUT(d_work, need, 0);
    HIP_OK(abi_stream(&st));
    uint32_t replies = 0;
    for (int round = 0; round < 3; ++round) {
        /* round 1: at most 100 replies; round 2: none, and no arrays */
        const uint32_t cap = round == 0 ? N : round == 1 ? 100 : 0;
        OUT(d_out, sizeof out, FILL);
        OUT(d_rs, sizeof rep_src, FILL);
        OUT(d_rl, sizeof rep_len8, FILL);
        OUT(d_acc, sizeof accept, FILL);
        OUT(d_conn, sizeof conn, FILL);
        OUT(d_count, sizeof count, FILL);
        CHECK(rns_rx_tcp_listen_pool_dev(d_pool, sizeof pool, LOG2, d_idx, NBUF, d_bf, d_len, N, L4, L6, d_meta, d_tbl, 2,
                                         cap ? d_iss : NULL, 0x20, d_add, cap ? d_out : NULL, cap, cap ? d_rs : NULL,
                                         cap ? d_rl : NULL, cap ? d_acc : NULL, d_count, d_conn, d_work, need, st) == RNS_OK,
              "rns_rx_tcp_listen_pool_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(out, d_out, sizeof out);
        DOWN(rep_src, d_rs, sizeof rep_src);
        DOWN(rep_len8, d_rl, sizeof rep_len8);
        DOWN(accept, d_acc, sizeof accept);
        DOWN(conn, d_conn, sizeof conn);
        DOWN(count, d_count, sizeof count);
        memset(opened, 0, sizeof opened);
        uint32_t R = 0, V = 0, A = 0, acc_written = 0;
        for (uint32_t i = 0; i < N; ++i) {
            if (kind[i] >= 4) {
                CHECK(conn[i] == 0, "round %d conn[%u] = %02x for a datagram that is no unmatched segment", round, i, conn[i]);
                continue;
            }
            const int v6 = peer[i] & 1, syn = kind[i] <= 1 && port[i] < 2;
            if (opened[peer[i]][port[i]]) {
                CHECK(conn[i] == (RNS_CONN_UNMATCHED | RNS_CONN_LATER), "round %d conn[%u] = %02x, not LATER", round, i, conn[i]);
                continue;
            }
            if (syn)
                opened[peer[i]][port[i]] = 1;
            const uint8_t cls = (uint8_t)(RNS_CONN_UNMATCHED | (syn ? RNS_CONN_SYN : RNS_CONN_RST));
            if (R >= cap) {
                CHECK(conn[i] == (cls | RNS_CONN_NOBUF), "round %d conn[%u] = %02x, not NOBUF", round, i, conn[i]);
            } else {
                CHECK(conn[i] == (cls | RNS_CONN_BUILT), "round %d conn[%u] = %02x, not %02x", round, i, conn[i], cls | RNS_CONN_BUILT);
                const uint32_t hl = build(v6, remote[i], meta[i].dport, meta[i].sport, syn ? iss[A] : 1, meta[i].seq + 1, syn, 0x20 + add + V);
                CHECK(rep_src[R] == i && rep_len8[R] == hl, "round %d reply %u: src %u len %u", round, R, rep_src[R], rep_len8[R]);
                CHECK(memcmp(out + 64 * R, want, hl) == 0, "round %d reply %u (datagram %u): the head differs", round, R, i);
                for (uint32_t b = hl; b < 64; ++b)
                    CHECK(out[64 * R + b] == FILL, "round %d reply %u: byte %u past its length written", round, R, b);
                if (syn) {
                    rns_tcp_accept w;
                    memset(&w, 0, sizeof w);
                    memcpy(w.key.ip, remote[i], v6 ? 16 : 4);
                    w.key.sport = meta[i].sport;
                    w.key.dport = meta[i].dport;
                    w.key.family = v6 ? 6 : 4;
                    w.flow.rcv_nxt = w.flow.rcv_max = meta[i].seq + 1;
                    w.flow.snd_una = w.flow.snd_wl1 = meta[i].seq;
                    w.flow.snd_nxt = iss[A];
                    w.flow.snd_wnd = meta[i].window;
                    w.flow.snd_wl2 = meta[i].ack;
                    w.flow.state = RNS_TCP_SYN_RECEIVED;
                    w.src = i;
                    w.listener = (uint16_t)port[i];
                    w.mss = kind[i] == 1 ? 1460 : 0;
                    CHECK(memcmp(&accept[A], &w, sizeof w) == 0, "round %d accept %u (datagram %u) differs", round, A, i);
                    acc_written = A + 1;
                }
            }
            R += 1;
            V += !v6;
            A += (uint32_t)syn;
        }
        CHECK(count[0] == R && count[1] == V && count[2] == A, "round %d counts %u %u %u, not %u %u %u", round, count[0], count[1],
              count[2], R, V, A);
        const uint8_t *ab = (const uint8_t *)accept;
        for (uint32_t r = R < cap ? R : cap; r < N; ++r)
            CHECK(rep_len8[r] == FILL && rep_src[r] == 0x55555555u && out[64 * r] == FILL && out[64 * r + 63] == FILL,
                  "round %d: slot %u written", round, r);
        for (size_t b = sizeof(rns_tcp_accept) * acc_written; b < sizeof accept; ++b)
            CHECK(ab[b] == FILL, "round %d: accept byte %zu written", round, b);
        replies = R;
    }
    CHECK(replies > 100, "the capped round cuts: %u replies", replies);
    /* no datagrams: the counts alone */
    OUT(d_count, sizeof count, FILL);
    CHECK(rns_rx_tcp_listen_pool_dev(NULL, 0, LOG2, NULL, 0, NULL, NULL, 0, L4, L6, NULL, NULL, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL,
                                     d_count, NULL, NULL, 0, st) == RNS_OK, "no datagrams");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(count, d_count, sizeof count);
    CHECK(count[0] == 0 && count[1] == 0 && count[2] == 0, "no datagrams: the counts are zeroed");
    return abi_finish("%d datagrams, %u replies", N, replies);
}
