/*
 * A plain C caller of the ICMP echo responder (rns_rx_icmp_echo_pool_dev, rns_rx_icmp_echo_work), bound
 * the way the reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the HIP
 * runtime only for device memory.  200 datagrams — echo requests over IPv4 (with and without options)
 * and IPv6, echo replies, UDP and a request with a corrupted checksum — lie in shuffled 512-byte pool
 * buffers as recv_packet leaves them.  The program builds the reply of every request itself (plain RFC
 * 1071 arithmetic over the bytes; icmp.rs:44-120, ip.rs:141-182), gathers the device's replies from the
 * transmit pool through the descriptors the call wrote — d_free is their buffer index — and compares
 * them byte for byte, with the flags, the counts, the ids (the base wraps) and the source indices;
 * then once more with too short a free list.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0xEC40F00Dull
#include "abi_test.h"

enum { N = 200, LOG2 = 9, BUF = 1 << LOG2, MAXPAY = 1400, MAXT = 60 + 4 + MAXPAY, MAXFR = 1 + (MAXT + BUF - 1) / BUF,
       NRX = N * MAXFR, NTX = N * MAXFR, NBLK = (N + 63) / 64, KINDS = 7, ID_BASE = 0xFFF0, ID_ADD = 5 };

static const uint8_t L4[4] = {10, 0, 0, 2}, R4[4] = {10, 0, 0, 1};
static const uint8_t L6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
static const uint8_t R6[16] = {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};

/* RFC 1071 over big-endian words, an odd last byte zero-padded; the folded sum */
static uint32_t be_sum(uint32_t s, const uint8_t *b, uint32_t n)
{
    for (uint32_t i = 0; i + 1 < n; i += 2)
        s += ((uint32_t)b[i] << 8) | b[i + 1];
    if (n & 1)
        s += (uint32_t)b[n - 1] << 8;
    while (s > 0xffff)
        s = (s & 0xffff) + (s >> 16);
    return s;
}

/* An ICMP datagram of `pay` random payload bytes: IPv4 with IHL ihl (v6 == 0) or IPv6.  Its length. */
static uint32_t make_icmp(uint8_t *d, int v6, uint32_t ihl, uint8_t type, uint32_t pay, int corrupt)
{
    const uint32_t h = v6 ? 40 : 4 * ihl, T = h + 4 + pay;
    memset(d, 0, h + 4);
    fill_random_bytes(d + h + 4, pay);
    d[h] = type;
    d[h + 1] = (uint8_t)next_u64();  /* the code is not echoed */
    uint32_t seed = 0;
    if (v6) {
        ipv6_header(d, 4 + pay, 58, R6, L6);
        seed = be_sum(be_sum(4 + pay + 58, R6, 16), L6, 16);
    } else {
        d[0] = (uint8_t)(0x40 | ihl); put16(d + 2, T); d[8] = 64; d[9] = 1;
        memcpy(d + 12, R4, 4); memcpy(d + 16, L4, 4);
        for (uint32_t b = 20; b < h; ++b)
            d[b] = 1;  /* options */
        put16(d + 10, be_sum(0, d, h) ^ 0xffff);
    }
    put16(d + h + 2, (be_sum(seed, d + h, 4 + pay) ^ 0xffff) ^ (corrupt ? 0x0100u : 0u));
    return T;
}

/* The reply to request d (ip header h bytes, T bytes in all) with IPv4 id `id`: its length. */
static uint32_t make_reply(uint8_t *r, const uint8_t *d, uint32_t h, uint32_t T, uint32_t id)
{
    const int v6 = (d[0] >> 4) == 6;
    const uint32_t pay = T - h - 4, hl = v6 ? 44 : 24;
    memset(r, 0, hl);
    memcpy(r + hl, d + h + 4, pay);
    uint32_t seed = 0;
    if (v6) {
        ipv6_header(r, 4 + pay, 58, L6, R6);
        r[40] = 129;
        seed = be_sum(be_sum(4 + pay + 58, R6, 16), L6, 16);
    } else {
        r[0] = 0x45; put16(r + 2, 24 + pay); put16(r + 4, id & 0xffff); r[8] = 64; r[9] = 1;
        memcpy(r + 12, L4, 4); memcpy(r + 16, R4, 4);
        put16(r + 10, be_sum(0, r, 20) ^ 0xffff);
    }
    put16(r + hl - 2, be_sum(seed, r + hl - 4, 4 + pay) ^ 0xffff);
    return hl + pay;
}

int main(void)
{
    static uint8_t rx[NRX * BUF], tx[NTX * BUF], back[NTX * BUF], dg[N][MAXT], want[MAXT], got[MAXT], status[N], echo[N], hl8[N];
    static uint16_t len16[N], pl16[N];
    static uint32_t idx[NRX], blk_first[NBLK], order[NRX], freel[NTX], tbf[NBLK], src[N], count[3], hdr[N];
    static int is_req[N];
    for (uint32_t j = 0; j < NRX; ++j)
        order[j] = freel[j] = j;
    for (uint32_t j = NRX - 1; j > 0; --j) {  /* pools whose buffers have been in use: any order */
        const uint32_t r = (uint32_t)(next_u64() % (j + 1)), t = order[j], r2 = (uint32_t)(next_u64() % (j + 1)), t2 = freel[j];
        order[j] = order[r];
        order[r] = t;
        freel[j] = freel[r2];
        freel[r2] = t2;
    }
    fill_random_bytes(rx, sizeof rx);
    memset(tx, 0xA5, sizeof tx);
    uint32_t nf = 0, nreq = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t edge[] = {0, 1, 15, 16, 17, BUF - 1, BUF, BUF + 1, MAXPAY};
        const uint32_t pay = i < 9 ? edge[i] : (uint32_t)(next_u64() % (MAXPAY + 1)), k = i % KINDS;
        uint32_t T;
        if (k == 4) {  /* UDP over IPv4 */
            T = make_icmp(dg[i], 0, 5, 8, pay + 4, 0);
            dg[i][9] = 17;
            put16(dg[i] + 10, 0);
            put16(dg[i] + 10, be_sum(0, dg[i], 20) ^ 0xffff);
        } else {
            T = make_icmp(dg[i], k == 1 || k == 5, k == 2 ? 5 + i % 11 : 5, k == 3 ? 0 : (k == 1 || k == 5) ? 128 : 8, pay, k == 6);
        }
        is_req[i] = k == 0 || k == 1 || k == 2 || k == 5;
        nreq += (uint32_t)is_req[i];
        hdr[i] = (dg[i][0] >> 4) == 6 ? 40 : 4u * (dg[i][0] & 15);
        len16[i] = (uint16_t)T;
        if ((i & 63) == 0)
            blk_first[i >> 6] = nf;
        for (uint32_t pos = 0; pos < T; pos += BUF, ++nf) {
            idx[nf] = order[nf];
            memcpy(rx + ((size_t)idx[nf] << LOG2), dg[i] + pos, T - pos < BUF ? T - pos : BUF);
        }
    }

    uint64_t need = 0, need0 = 0;
    CHECK(rns_rx_icmp_echo_work(N, NULL) == RNS_E_INVALID, "NULL bytes");
    CHECK(rns_rx_icmp_echo_work(0, &need0) == RNS_OK && need0 > 0, "work(0)");
    CHECK(rns_rx_icmp_echo_work(N, &need) == RNS_OK && need >= need0, "work(N)");
    /* argument checks need no device */
    uint8_t *fake = (uint8_t *)4096;
#define CALL(rxp, log2, txp, cnt, wk, wkb)                                                                              \
    rns_rx_icmp_echo_pool_dev(rxp, sizeof rx, log2, (uint32_t *)fake, nf, (uint32_t *)fake, (uint16_t *)fake, N, L4, L6, txp, \
                              sizeof tx, (uint32_t *)fake, NTX, N, 0, NULL, (uint32_t *)fake, fake, (uint16_t *)fake, NULL,  \
                              cnt, fake, NULL, fake, wk, wkb, NULL)
    CHECK(CALL(fake, 7, fake, (uint32_t *)fake, fake, need) == RNS_E_INVALID, "buf_log2 7");
    CHECK(CALL(fake + 8, LOG2, fake, (uint32_t *)fake, fake, need) == RNS_E_INVALID, "a misaligned receive pool");
    CHECK(CALL(fake, LOG2, NULL, (uint32_t *)fake, fake, need) == RNS_E_INVALID, "NULL transmit pool");
    CHECK(CALL(fake, LOG2, fake, NULL, fake, need) == RNS_E_INVALID, "NULL counts");
    CHECK(CALL(fake, LOG2, fake, (uint32_t *)fake, fake, need - 1) == RNS_E_INVALID, "a short workspace");

    uint8_t *d_rx = NULL, *d_tx = NULL, *d_status = NULL, *d_echo = NULL, *d_hl = NULL;
    uint16_t *d_len = NULL, *d_pl = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL, *d_free = NULL, *d_tbf = NULL, *d_src = NULL, *d_count = NULL, *d_add = NULL;
    void *d_work = NULL;
    hipStream_t st;
    const uint32_t add = ID_ADD;
    UP(d_rx, rx, sizeof rx);
    UP(d_len, len16, sizeof len16);
    UP(d_idx, idx, sizeof idx);
    UP(d_blk, blk_first, sizeof blk_first);
    UP(d_free, freel, sizeof freel);
    UP(d_add, &add, 4);
    OUT(d_status, N, 0);
    OUT(d_echo, N, 0);
    OUT(d_hl, N, 0);
    OUT(d_pl, sizeof pl16, 0);
    OUT(d_tbf, sizeof tbf, 0);
    OUT(d_src, sizeof src, 0);
    OUT(d_work, need, 0);
    HIP_OK(abi_stream(&st));
    for (int round = 0; round < 2; ++round) {
        /* round 1: a free list that ends inside the 21st reply: 20 replies, the other requests left to the host */
        uint32_t n_free = NTX, want_rep = nreq;
        if (round == 1) {
            n_free = 0;
            want_rep = 20;
            for (uint32_t i = 0, r = 0; r <= want_rep; ++i)
                if (is_req[i]) {
                    n_free += 1u + (len16[i] - hdr[i] - 4u + BUF - 1u) / BUF;
                    ++r;
                }
            n_free -= 1;
        }
        UP(d_tx, tx, sizeof tx);
        OUT(d_count, sizeof count, 0x55);
        CHECK(rns_rx_icmp_echo_pool_dev(d_rx, sizeof rx, LOG2, d_idx, nf, d_blk, d_len, N, L4, L6, d_tx, sizeof tx, d_free, n_free,
                                        N, ID_BASE, d_add, d_tbf, d_hl, d_pl, d_src, d_count, d_status, NULL, d_echo, d_work,
                                        need, st) == RNS_OK, "rns_rx_icmp_echo_pool_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(count, d_count, sizeof count);
        DOWN(status, d_status, N);
        DOWN(echo, d_echo, N);
        DOWN(hl8, d_hl, N);
        DOWN(pl16, d_pl, sizeof pl16);
        DOWN(tbf, d_tbf, sizeof tbf);
        DOWN(src, d_src, sizeof src);
        DOWN(back, d_tx, sizeof tx);
        CHECK(count[0] == want_rep, "round %d: %u replies, %u expected", round, count[0], want_rep);
        uint32_t r = 0, at = 0, v4 = 0;
        for (uint32_t i = 0; i < N; ++i) {
            const uint8_t e = !is_req[i] ? 0 : r < want_rep ? RNS_ECHO_REQUEST | RNS_ECHO_BUILT : RNS_ECHO_REQUEST | RNS_ECHO_NOBUF;
            CHECK(echo[i] == e, "round %d echo[%u] = %02x, not %02x", round, i, echo[i], e);
            CHECK(((status[i] & RNS_RX_ACCEPT) != 0) == (i % KINDS != 6), "status[%u] = %02x", i, status[i]);
            if (e != (RNS_ECHO_REQUEST | RNS_ECHO_BUILT) || r >= count[0])
                continue;
            const int v6 = (dg[i][0] >> 4) == 6;
            const uint32_t len = make_reply(want, dg[i], hdr[i], len16[i], ID_BASE + ID_ADD + v4), pay = len - (v6 ? 44 : 24);
            v4 += !v6;
            if ((r & 63) == 0) {
                CHECK(tbf[r >> 6] == at, "round %d tx_blk_first[%u]", round, r >> 6);
                at = tbf[r >> 6];
            }
            CHECK(src[r] == i && hl8[r] == (v6 ? 44 : 24) && pl16[r] == pay, "round %d reply %u: src %u head %u pay %u", round, r,
                  src[r], hl8[r], pl16[r]);
            /* gather: the head at its buffer's end, then the payload buffers, all named by d_free */
            if (at + 1 + (pay + BUF - 1) / BUF <= n_free && hl8[r] <= 44) {
                memcpy(got, back + ((size_t)freel[at] << LOG2) + BUF - hl8[r], hl8[r]);
                for (uint32_t pos = 0, f = at + 1; pos < pay; pos += BUF, ++f)
                    memcpy(got + hl8[r] + pos, back + ((size_t)freel[f] << LOG2), pay - pos < BUF ? pay - pos : BUF);
                CHECK(memcmp(got, want, len) == 0, "round %d reply %u (datagram %u) differs", round, r, i);
            }
            at += 1 + (pay + BUF - 1) / BUF;
            ++r;
        }
        CHECK(count[1] == at && count[2] == v4, "round %d counts %u %u, expected %u %u", round, count[1], count[2], at, v4);
        for (uint32_t f = at; f < NTX; ++f)  /* buffers that were not taken are untouched */
            for (uint32_t b = 0; b < BUF; b += 61)
                CHECK(back[((size_t)freel[f] << LOG2) + b] == 0xA5, "round %d: free buffer %u written", round, f);
    }
    return abi_finish("%d datagrams, %u echo requests", N, nreq);
}
