/*
 * A plain C caller of the transmit finalize over pool buffers (rns_tx_fill_pool_dev) and its host
 * layout helper (rns_tx_pool_layout), bound the way the reference's Rust would bind them (extern "C"
 * + raw pointers): no torch, no Python, the HIP runtime only for device memory.  300 datagrams —
 * TCP, UDP and ICMP over IPv4, TCP over IPv6, head-only ones, a head with one payload byte in it, an
 * empty head and an unknown IP version — lie in shuffled 512-byte pool buffers as the reference's
 * transmit path leaves them (the head at its buffer's end, buf.rs:262-291; the payload in whole
 * buffers and a last partly filled one, buf.rs:385-420).  Every pool byte and every status is checked
 * against oracle_tx_chain_fill (oracle/csum_oracle.c, linked as test infrastructure only) on the CSR
 * chains the compact form expands to, first as laid out and then with one index outside the pool.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x7001F00Dull
#include "abi_test.h"

enum { N = 300, LOG2 = 9, BUF = 1 << LOG2, MAXPAY = 2000, MAXFR = 1 + (MAXPAY + BUF - 1) / BUF, NBUF = N * MAXFR,
       NBLK = (N + 63) / 64, KINDS = 7, EMPTY_HEAD = 131, OUTSIDE = 201 };

/* The head of a datagram of kind k over a payload of `pay` bytes: its length.  The fields the
 * finalize computes hold random bytes (they count as zero). */
static uint32_t make_head(uint8_t *h, int k, uint32_t pay)
{
    static const uint32_t hlen[KINDS] = {40, 60, 28, 28, 40, 41, 40};
    const uint32_t hl = hlen[k];
    fill_random_bytes(h, hl);
    if (k == 1) {  /* IPv6, TCP */
        h[0] = 0x60; put16(h + 4, pay + 20); h[6] = 6; h[7] = 64;
    } else {       /* IPv4: TCP, UDP (2), ICMP (3), TCP with a payload byte in the head (5), version 7 (6) */
        h[0] = k == 6 ? 0x75 : 0x45; put16(h + 2, hl + pay); h[6] = 0x40; h[7] = 0; h[8] = 64;
        h[9] = k == 2 ? 17 : k == 3 ? 1 : 6;
    }
    return hl;
}

int main(void)
{
    static uint8_t pool[NBUF * BUF], want[NBUF * BUF], back[NBUF * BUF], head[64], status[N], want_st[N], hl8[N];
    static uint16_t pl16[N];
    static uint32_t idx[NBUF], blk_first[NBLK], first[N + 1], frag_len[NBUF], order[NBUF];
    static uint64_t frag_off[NBUF];
    shuffled_order(order, NBUF);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t edge[] = {0, 1, 2, BUF - 1, BUF, BUF + 1, 2 * BUF, 2 * BUF + 1, MAXPAY};
        pl16[i] = (uint16_t)(i % KINDS == 4 ? 0 : i < 9 ? edge[i] : next_u64() % (MAXPAY + 1));
    }

    /* the layout helper: the index of the compact form and of the chains it expands to */
    uint64_t nf64 = 0;
    CHECK(rns_tx_pool_layout(pl16, N, 7, blk_first, first, &nf64) == RNS_E_INVALID, "buf_log2 7");
    CHECK(rns_tx_pool_layout(pl16, N, 16, blk_first, first, &nf64) == RNS_E_INVALID, "buf_log2 16");
    CHECK(rns_tx_pool_layout(pl16, N, LOG2, blk_first, first, NULL) == RNS_E_INVALID, "NULL n_frags");
    CHECK(rns_tx_pool_layout(pl16, N, LOG2, blk_first, first, &nf64) == RNS_OK, "layout");
    const uint32_t nf = (uint32_t)nf64;
    CHECK(first[0] == 0 && first[N] == nf && nf <= NBUF, "first[0], first[N] = %u, %u", first[0], first[N]);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(first[i + 1] - first[i] == 1u + (pl16[i] + BUF - 1u) / BUF, "buffers of datagram %u", i);
        CHECK((i & 63) || blk_first[i >> 6] == first[i], "blk_first[%u]", i >> 6);
    }

    fill_random_bytes(pool, sizeof pool);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t pay = pl16[i];
        uint32_t hl = make_head(head, (int)(i % KINDS), pay);
        if (i == EMPTY_HEAD)
            hl = 0;
        hl8[i] = (uint8_t)hl;
        uint32_t f = first[i];
        idx[f] = order[f];
        frag_off[f] = ((uint64_t)idx[f] << LOG2) + BUF - hl;
        frag_len[f] = hl;
        memcpy(pool + frag_off[f], head, hl);
        for (uint32_t pos = 0; pos < pay; pos += BUF) {  /* the payload bytes are the pool's random ones */
            ++f;
            idx[f] = order[f];
            frag_off[f] = (uint64_t)idx[f] << LOG2;
            frag_len[f] = pay - pos < BUF ? pay - pos : BUF;
        }
        CHECK(f + 1 == first[i + 1], "datagram %u fills its buffers", i);
    }
    memcpy(want, pool, sizeof pool);
    oracle_tx_chain_fill(want, sizeof pool, frag_off, frag_len, first, nf, N, want_st);
    int filled = 0, malformed = 0;
    for (uint32_t i = 0; i < N; ++i) {
        filled += want_st[i] == (RNS_TX_IP_FILLED | RNS_TX_L4_FILLED);
        malformed += want_st[i] == RNS_TX_MALFORMED;
    }
    CHECK(want_st[EMPTY_HEAD] == RNS_TX_MALFORMED && malformed == 1 + (N + 0) / KINDS && filled > N / 2,
          "the oracle: %d filled, %d malformed", filled, malformed);

    /* argument checks need no device */
    CHECK(rns_tx_fill_pool_dev(NULL, 0, 0, NULL, 0, NULL, NULL, NULL, 0, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_tx_fill_pool_dev(pool, sizeof pool, 7, idx, nf, blk_first, hl8, pl16, N, status, NULL) == RNS_E_INVALID,
          "buf_log2 7");
    CHECK(rns_tx_fill_pool_dev(pool, sizeof pool, LOG2, NULL, nf, blk_first, hl8, pl16, N, status, NULL) == RNS_E_INVALID,
          "NULL indices");
    CHECK(rns_tx_fill_pool_dev(pool, sizeof pool, LOG2, idx, nf, blk_first, NULL, pl16, N, status, NULL) == RNS_E_INVALID,
          "NULL head lengths");

    uint8_t *d_pool = NULL, *d_status = NULL, *d_hl = NULL;
    uint16_t *d_pl = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL;
    hipStream_t st;
    UP(d_hl, hl8, N);
    UP(d_pl, pl16, N * sizeof *pl16);
    UP(d_blk, blk_first, NBLK * sizeof *blk_first);
    HIP_OK(abi_stream(&st));
    for (int round = 0; round < 2; ++round) {
        if (round == 1) {  /* one index outside the pool: that datagram alone is rejected, untouched */
            const uint32_t f = first[OUTSIDE] + 1;
            CHECK(first[OUTSIDE + 1] > f && want_st[OUTSIDE] != RNS_TX_MALFORMED, "datagram %d has a payload", OUTSIDE);
            idx[f] = NBUF + 5;
            frag_off[f] = (uint64_t)idx[f] << LOG2;
            memcpy(want, pool, sizeof pool);
            oracle_tx_chain_fill(want, sizeof pool, frag_off, frag_len, first, nf, N, want_st);
            CHECK(want_st[OUTSIDE] == RNS_TX_MALFORMED, "the oracle rejects the index outside the pool");
        }
        UP(d_pool, pool, sizeof pool);
        UP(d_idx, idx, NBUF * sizeof *idx);
        OUT(d_status, N, 0x55);
        CHECK(rns_tx_fill_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_hl, d_pl, N, d_status, st) == RNS_OK,
              "rns_tx_fill_pool_dev");
        HIP_OK(hipStreamSynchronize(st));
        DOWN(status, d_status, N);
        DOWN(back, d_pool, sizeof pool);
        for (uint32_t i = 0; i < N; ++i)
            CHECK(status[i] == want_st[i], "round %d status %u: %02x != %02x", round, i, status[i], want_st[i]);
        for (size_t b = 0; b < sizeof pool; ++b)
            CHECK(back[b] == want[b], "round %d pool byte %zu: %02x != %02x", round, b, back[b], want[b]);
    }
    /* without the status array: the same bytes */
    UP(d_pool, pool, sizeof pool);
    CHECK(rns_tx_fill_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_hl, d_pl, N, NULL, st) == RNS_OK,
          "no status array");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(back, d_pool, sizeof pool);
    CHECK(memcmp(back, want, sizeof pool) == 0, "without the status array: the pool differs");
    return abi_finish("%d datagrams in %u pool buffers", N, nf);
}
