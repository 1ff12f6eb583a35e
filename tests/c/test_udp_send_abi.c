/*
 * A plain C caller of the UDP send build (rns_tx_udp_send_pool_dev, rns_tx_udp_send_work), bound the way the
 * reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the HIP runtime only for
 * device memory.  1000 sends from 12 sockets (two of them empty) to IPv4 and IPv6 peers, grouped by socket
 * as udp_send is called, their payloads 16-byte aligned in one array; some records are no sends (not queued,
 * a bad family, a payload past the array, records past d_q_first's total).  The program builds every datagram
 * itself the way udp_output and ip_output do (udp.rs:150-173, ip.rs:140-177) over a flat copy, then compares the
 * heads at the end of their head buffers, every payload byte, the descriptors, d_send and d_count, and that no
 * buffer but the datagrams' own is written; then once more with a send cap, and with a short free list.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x5E4DF00Dull
#include "abi_test.h"

enum { N = 1000, NREC = N + 24, LOG2 = 9, BUF = 1 << LOG2, MAXPAY = 1300, MAXFR = 1 + (MAXPAY + BUF - 1) / BUF, NTX = N * MAXFR + 7,
       SOCKS = 12, DATA = N * ((MAXPAY + 15) / 16 * 16) };

static const uint8_t L4[4] = {10, 0, 0, 2}, R4[4] = {10, 0, 0, 1};
static const uint8_t L6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
static const uint8_t R6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};

static uint8_t data[DATA], tx[NTX * BUF], tx0[NTX * BUF], send[NREC], head_len8[NREC], want[48 + MAXPAY];
static uint16_t pay_len16[NREC], ports[SOCKS];
static uint32_t q_first[SOCKS + 1], freel[NTX], blk_first[(NREC + 63) / 64], src[NREC], count[3], sock_of[NREC];
static rns_udp_rec rec[NREC];

/* udp_output and ip_output over a flat copy: the head (28 / 48 bytes) then the payload, in `want`.  The head's length. */
static uint32_t build(const rns_udp_rec *r, uint16_t port, uint32_t id)
{
    const int v6 = r->family == 6;
    const uint32_t h = v6 ? 40 : 20, len = r->len;
    memset(want, 0, h + 8);
    memcpy(want + h + 8, data + 16ull * r->off16, len);
    put16(want + h, port);
    put16(want + h + 2, r->sport);
    put16(want + h + 4, 8 + len);
    l4_checksum(want + h, 8 + len, 6, v6 ? L6 : L4, r->ip, v6 ? 16 : 4, 17);
    if (v6) {
        ipv6_header(want, 8 + len, 17, L6, r->ip);
    } else {
        want[0] = 0x45; put16(want + 2, 28 + len); put16(want + 4, id); want[8] = 64; want[9] = 17;
        memcpy(want + 12, L4, 4);
        memcpy(want + 16, r->ip, 4);
        ipv4_checksum(want, 20);
    }
    return h + 8;
}

int main(void)
{
    /* the sockets' sizes: sockets 4 and 11 are empty */
    uint32_t size[SOCKS] = {0};
    for (uint32_t k = 0; k < N; ++k) {
        uint32_t s = (uint32_t)(next_u64() % SOCKS);
        size[s == 4 || s == 11 ? 0 : s]++;
    }
    for (uint32_t s = 0, at = 0; s <= SOCKS; ++s) {
        q_first[s] = at;
        if (s < SOCKS) {
            ports[s] = (uint16_t)(7000 + 13 * s);
            for (uint32_t j = 0; j < size[s]; ++j)
                sock_of[at + j] = s;
            at += size[s];
        }
    }
    fill_random_bytes(data, sizeof data);
    uint32_t off16 = 0, nsend = 0;
    uint8_t is_send[NREC];
    for (uint32_t k = 0; k < NREC; ++k) {
        const uint32_t edge[] = {0, 1, 15, 16, 17, BUF - 1, BUF, BUF + 1, 2 * BUF, 2 * BUF + 1, MAXPAY};
        const uint32_t len = k < 11 ? edge[k] : (uint32_t)(next_u64() % (k % 3 ? 90 : MAXPAY));
        const int v6 = (k % 5 == 1 || k % 5 == 3);
        memset(&rec[k], 0, sizeof rec[k]);
        memcpy(rec[k].ip, v6 ? R6 : R4, v6 ? 16 : 4);
        rec[k].ip[v6 ? 15 : 3] = (uint8_t)(1 + k % 200);
        rec[k].src = 0xABCD0000u + k;  /* not read */
        rec[k].pad[0] = rec[k].pad[1] = 0xEE;
        rec[k].off16 = off16;
        rec[k].sport = (uint16_t)(1024 + next_u64() % 60000);
        rec[k].len = (uint16_t)len;
        rec[k].family = v6 ? 6 : 4;
        rec[k].flags = RNS_UDP_DGRAM | RNS_UDP_SOCK | RNS_UDP_QUEUED;
        is_send[k] = k < N;                        /* records N.. lie past d_q_first[SOCKS] */
        if (k < N) {
            off16 += (len + 15) / 16;
            if (k % 97 == 50) { rec[k].flags = RNS_UDP_DGRAM | RNS_UDP_SOCK | RNS_UDP_NOROOM; is_send[k] = 0; }
            if (k % 97 == 60) { rec[k].family = 0; is_send[k] = 0; }
            if (k % 97 == 70) { rec[k].off16 = DATA / 16 + 1; is_send[k] = 0; }  /* a payload past the array */
        }
        nsend += is_send[k];
    }
    CHECK(16ull * off16 <= DATA, "the payloads fit");
    shuffled_order(freel, NTX);
    fill_random_bytes(tx0, sizeof tx0);

    /* the workspace size and every argument check need no device */
    uint64_t need = 0, need0 = 0;
    CHECK(rns_tx_udp_send_work(N, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_tx_udp_send_work(RNS_CHAIN_MAX_PACKETS + 1, &need) == RNS_E_INVALID, "too many records for the workspace");
    CHECK(rns_tx_udp_send_work(0, &need0) == RNS_OK && need0 > 0, "work(0)");
    CHECK(rns_tx_udp_send_work(NREC, &need) == RNS_OK && need >= need0, "work(NREC)");
    uint8_t *fake = (uint8_t *)4096;
    uint32_t *const f32 = (uint32_t *)fake;
    uint16_t *const f16 = (uint16_t *)fake;
    rns_udp_rec *const frec = (rns_udp_rec *)fake;
#define CALL(dt, rc, n, qf, sp, ns, l4, l6, pool, log2, fr, nfree, cap, bf, hl, pl, cnt, sd, wk, wkb)                                \
    rns_tx_udp_send_pool_dev(dt, DATA, rc, n, qf, sp, ns, l4, l6, pool, sizeof tx, log2, fr, nfree, cap, 0, NULL, bf, hl, pl, NULL, cnt, \
                             sd, wk, wkb, NULL)
#define BAD(what, ...) CHECK(CALL(__VA_ARGS__) == RNS_E_INVALID, what)
    BAD("NULL data", NULL, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("misaligned data", fake + 8, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL records", fake, NULL, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("misaligned records", fake, (rns_udp_rec *)(fake + 8), N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("too many records", fake, frec, RNS_CHAIN_MAX_PACKETS + 1, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, ~0ull);
    BAD("NULL q_first", fake, frec, N, NULL, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL ports", fake, frec, N, f32, NULL, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("no sockets", fake, frec, N, f32, f16, 0, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("too many sockets", fake, frec, N, f32, f16, RNS_UDP_MAX_SOCKS + 1, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL IPv4 address", fake, frec, N, f32, f16, SOCKS, NULL, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL IPv6 address", fake, frec, N, f32, f16, SOCKS, L4, NULL, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL pool", fake, frec, N, f32, f16, SOCKS, L4, L6, NULL, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("misaligned pool", fake, frec, N, f32, f16, SOCKS, L4, L6, fake + 8, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("buf_log2 7", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, 7, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("buf_log2 16", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, 16, f32, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL free list", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, NULL, NTX, N, f32, fake, f16, f32, fake, fake, need);
    BAD("NULL tx_blk_first", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, NULL, fake, f16, f32, fake, fake, need);
    BAD("NULL tx_head_len8", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, NULL, f16, f32, fake, fake, need);
    BAD("NULL tx_pay_len16", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, NULL, f32, fake, fake, need);
    BAD("NULL counts", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, NULL, fake, fake, need);
    BAD("NULL d_send", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, NULL, fake, need);
    BAD("NULL workspace", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, NULL, need);
    BAD("a misaligned workspace", fake, frec, N, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake + 4, need);
    BAD("a short workspace", fake, frec, NREC, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, f32, fake, fake, need - 1);
    BAD("no records, NULL counts", fake, frec, 0, f32, f16, SOCKS, L4, L6, fake, LOG2, f32, NTX, N, f32, fake, f16, NULL, fake, fake, need);

    uint8_t *d_data = NULL, *d_tx = NULL, *d_send = NULL, *d_hl = NULL;
    uint16_t *d_ports = NULL, *d_pl = NULL;
    uint32_t *d_qf = NULL, *d_free = NULL, *d_bf = NULL, *d_src = NULL, *d_count = NULL, *d_add = NULL;
    rns_udp_rec *d_rec = NULL;
    void *d_work = NULL;
    hipStream_t st;
    const uint32_t add = 0x2fff0;  /* with the base: the ids wrap */
    UP(d_data, data, sizeof data);
    UP(d_rec, rec, sizeof rec);
    UP(d_qf, q_first, sizeof q_first);
    UP(d_ports, ports, sizeof ports);
    UP(d_free, freel, sizeof freel);
    UP(d_add, &add, sizeof add);
    OUT(d_work, need, 0);
    HIP_OK(abi_stream(&st));
    for (int round = 0; round < 3; ++round) {
        /* round 1: at most 300 datagrams; round 2: 500 free buffers */
        const uint32_t cap = round == 1 ? 300 : NREC, nfree = round == 2 ? 500 : NTX;
        UP(d_tx, tx0, sizeof tx0);
        OUT(d_send, NREC, 0x55);
        OUT(d_hl, NREC, 0x55);
        OUT(d_pl, sizeof pay_len16, 0x55);
        OUT(d_bf, sizeof blk_first, 0x55);
        OUT(d_src, sizeof src, 0x55);
        OUT(d_count, sizeof count, 0x55);
        CHECK(rns_tx_udp_send_pool_dev(d_data, DATA, d_rec, NREC, d_qf, d_ports, SOCKS, L4, L6, d_tx, sizeof tx, LOG2, d_free, nfree, cap,
                                       0x20, d_add, d_bf, d_hl, d_pl, d_src, d_count, d_send, d_work, need, st) == RNS_OK,
              "rns_tx_udp_send_pool_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(tx, d_tx, sizeof tx);
        DOWN(send, d_send, NREC);
        DOWN(head_len8, d_hl, NREC);
        DOWN(pay_len16, d_pl, sizeof pay_len16);
        DOWN(blk_first, d_bf, sizeof blk_first);
        DOWN(src, d_src, sizeof src);
        DOWN(count, d_count, sizeof count);
        static uint8_t own[NTX];
        memset(own, 0, sizeof own);
        uint32_t R = 0, F = 0, V = 0;
        int full = 0;
        for (uint32_t k = 0; k < NREC; ++k) {
            if (!is_send[k]) {
                CHECK(send[k] == 0, "round %d send[%u] = %02x for a record that is no send", round, k, send[k]);
                continue;
            }
            const uint32_t len = rec[k].len, nf = 1 + (len + BUF - 1) / BUF;
            if (full || R + 1 > cap || F + nf > nfree) {
                full = 1;
                CHECK(send[k] == (RNS_UDPTX_SEND | RNS_UDPTX_NOBUF), "round %d send[%u] = %02x, not NOBUF", round, k, send[k]);
                continue;
            }
            CHECK(send[k] == (RNS_UDPTX_SEND | RNS_UDPTX_BUILT), "round %d send[%u] = %02x, not BUILT", round, k, send[k]);
            const uint32_t hl = build(&rec[k], ports[sock_of[k]], 0x20 + add + V);
            CHECK(head_len8[R] == hl && pay_len16[R] == len && src[R] == k, "round %d datagram %u: head %u pay %u src %u", round, R,
                  head_len8[R], pay_len16[R], src[R]);
            if (R % 64 == 0)
                CHECK(blk_first[R / 64] == F, "round %d blk_first[%u] = %u, not %u", round, R / 64, blk_first[R / 64], F);
            const uint8_t *hb = tx + ((size_t)freel[F] << LOG2);
            CHECK(memcmp(hb + BUF - hl, want, hl) == 0, "round %d datagram %u (record %u): the head differs", round, R, k);
            CHECK(memcmp(hb, tx0 + ((size_t)freel[F] << LOG2), BUF - hl) == 0, "round %d datagram %u: written before its head", round, R);
            own[freel[F]] = 1;
            for (uint32_t j = 0; j + 1 < nf; ++j) {
                const uint32_t part = len - j * BUF < BUF ? len - j * BUF : BUF, b = freel[F + 1 + j], slack = (part + 15) / 16 * 16;
                CHECK(memcmp(tx + ((size_t)b << LOG2), want + hl + j * BUF, part) == 0, "round %d datagram %u: payload buffer %u differs", round, R, j);
                CHECK(memcmp(tx + ((size_t)b << LOG2) + slack, tx0 + ((size_t)b << LOG2) + slack, BUF - slack) == 0,
                      "round %d datagram %u: written past its payload's last 16-byte unit", round, R);
                own[b] = 1;
            }
            V += rec[k].family == 4;
            R += 1;
            F += nf;
        }
        CHECK(count[0] == R && count[1] == F && count[2] == V, "round %d counts %u %u %u, not %u %u %u", round, count[0], count[1],
              count[2], R, F, V);
        CHECK(round != 0 || R == nsend, "round 0 builds every send: %u of %u", R, nsend);
        for (uint32_t r = R; r < NREC; ++r)
            CHECK(head_len8[r] == 0x55 && pay_len16[r] == 0x5555 && src[r] == 0x55555555u, "round %d: descriptor %u written", round, r);
        for (uint32_t b = 0; b < NTX; ++b)
            if (!own[b])
                CHECK(memcmp(tx + ((size_t)b << LOG2), tx0 + ((size_t)b << LOG2), BUF) == 0, "round %d: buffer %u is no datagram's and was written",
                      round, b);
    }
    /* no records: the counts alone */
    OUT(d_count, sizeof count, 0x55);
    CHECK(rns_tx_udp_send_pool_dev(NULL, 0, NULL, 0, NULL, NULL, 0, L4, L6, NULL, 0, LOG2, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, d_count,
                                   NULL, NULL, 0, st) == RNS_OK, "no records");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(count, d_count, sizeof count);
    CHECK(count[0] == 0 && count[1] == 0 && count[2] == 0, "no records: the counts are zeroed");
    return abi_finish("%d records, %u sends from %d sockets", NREC, nsend, SOCKS);
}
