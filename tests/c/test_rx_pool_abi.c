/*
 * A plain C caller of the receive verify over pool buffers (rns_rx_verify_pool_dev) and its host
 * layout helper (rns_rx_pool_layout), bound the way the reference's Rust would bind them (extern "C"
 * + raw pointers): no torch, no Python, the HIP runtime only for device memory.  150 datagrams —
 * IPv4 TCP, IPv6 TCP and IPv4 ICMP, every fifth with a flipped byte, one of them empty — lie in
 * shuffled 512-byte pool buffers as recv_packet leaves them (netif.rs:65-83).  Every status and L4
 * value is checked against the receive path restated here over the oracle's primitives
 * (oracle/csum_oracle.c, linked as test infrastructure only) and against rns_rx_verify_chain_dev on
 * the CSR chains the compact form expands to.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x9001F00Dull
#include "abi_test.h"

enum { N = 150, LOG2 = 9, BUF = 1 << LOG2, MAXLEN = 2048, MAXFR = MAXLEN / BUF, NBUF = N * MAXFR, NBLK = (N + 63) / 64,
       EMPTY = 77 };

static const uint8_t local4[4] = {10, 0, 0, 2}, remote4[4] = {10, 0, 0, 1};
static const uint8_t local6[16] = {0xfd, [15] = 2}, remote6[16] = {0xfd, [15] = 1};
static const rx_addrs addrs = {remote4, local4, remote6, local6};

int main(void)
{
    static uint8_t pool[NBUF * BUF], dgram[MAXLEN], status[N], chain_status[N], ref_status[N];
    static uint16_t len16[N], l4[N], chain_l4[N], ref_l4[N];
    static uint32_t idx[NBUF], blk_first[NBLK], first[N + 1], frag_len[NBUF], order[NBUF];
    static uint64_t frag_off[NBUF];
    shuffled_order(order, NBUF);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t hdr = i % 3 == 1 ? 40 : 20;
        const uint32_t edge[] = {BUF - 1, BUF, BUF + 1, 2 * BUF, 2 * BUF + 1, MAXLEN, hdr + 20};
        len16[i] = (uint16_t)(i == EMPTY ? 0 : i < 7 ? edge[i] : hdr + 20 + next_u64() % (MAXLEN - hdr - 20 + 1));
    }

    /* the layout helper: the index of the compact form and of the chains it expands to */
    uint64_t nf64 = 0;
    CHECK(rns_rx_pool_layout(len16, N, 5, blk_first, first, &nf64) == RNS_E_INVALID, "buf_log2 5");
    CHECK(rns_rx_pool_layout(len16, N, LOG2, blk_first, first, NULL) == RNS_E_INVALID, "NULL n_frags");
    CHECK(rns_rx_pool_layout(len16, N, LOG2, blk_first, first, &nf64) == RNS_OK, "layout");
    const uint32_t nf = (uint32_t)nf64;
    CHECK(first[0] == 0 && first[N] == nf && nf <= NBUF, "first[0], first[N] = %u, %u", first[0], first[N]);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(first[i + 1] - first[i] == (len16[i] + BUF - 1u) / BUF, "fragments of datagram %u", i);
        CHECK((i & 63) || blk_first[i >> 6] == first[i], "blk_first[%u]", i >> 6);
    }

    memset(pool, 0xEE, sizeof pool);
    int accepted = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const int k = (int)(i % 3);
        const uint32_t hdr = k == 1 ? 40 : 20, dl = len16[i];
        if (dl) {
            make_datagram(dgram, dl, k, &addrs);
            if (i % 5 == 4)
                dgram[hdr + (next_u64() % (dl - hdr))] ^= 0x10;
        }
        for (uint32_t f = first[i], pos = 0; f < first[i + 1]; ++f, pos += BUF) {
            idx[f] = order[f];
            frag_off[f] = (uint64_t)idx[f] << LOG2;
            frag_len[f] = dl - pos < BUF ? dl - pos : BUF;
            memcpy(pool + frag_off[f], dgram + pos, frag_len[f]);
        }
        rx_reference_pool(pool, LOG2, idx + first[i], dl, local4, local6, &ref_status[i], &ref_l4[i]);
        accepted += (ref_status[i] & RNS_RX_ACCEPT) != 0;
    }
    CHECK(accepted == N - N / 5 - 1, "the oracle accepts %d of %d", accepted, N);
    CHECK(ref_status[EMPTY] == RNS_RX_MALFORMED, "the empty datagram");

    /* argument checks need no device */
    CHECK(rns_rx_verify_pool_dev(NULL, 0, 0, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, LOG2, idx, nf, blk_first, len16, N, local4, local6, NULL, NULL, NULL) ==
              RNS_E_INVALID, "NULL status");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, 16, idx, nf, blk_first, len16, N, local4, local6, status, NULL, NULL) ==
              RNS_E_INVALID, "buf_log2 16");
    CHECK(rns_rx_verify_pool_dev(pool, sizeof pool, LOG2, NULL, nf, blk_first, len16, N, local4, local6, status, NULL,
                                 NULL) == RNS_E_INVALID, "NULL indices");

    uint8_t *d_pool = NULL, *d_status = NULL;
    uint16_t *d_l4 = NULL, *d_len16 = NULL;
    uint64_t *d_off = NULL;
    uint32_t *d_idx = NULL, *d_blk = NULL, *d_len = NULL, *d_first = NULL;
    hipStream_t st;
    UP(d_pool, pool, sizeof pool);
    UP(d_len16, len16, N * sizeof *len16);
    UP(d_idx, idx, NBUF * sizeof *idx);
    UP(d_blk, blk_first, NBLK * sizeof *blk_first);
    UP(d_off, frag_off, NBUF * sizeof *frag_off);
    UP(d_len, frag_len, NBUF * sizeof *frag_len);
    UP(d_first, first, (N + 1) * sizeof *first);
    OUT(d_status, N, 0x55);
    OUT(d_l4, N * sizeof *l4, 0);
    HIP_OK(abi_stream(&st));
    CHECK(rns_rx_verify_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_status, d_l4,
                                 st) == RNS_OK, "rns_rx_verify_pool_dev");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(status, d_status, N);
    DOWN(l4, d_l4, N * sizeof *l4);
    /* the existing entry on the expanded chains, over the same pool */
    OUT(d_status, N, 0x55);
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, d_l4, st) ==
              RNS_OK, "rns_rx_verify_chain_dev");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(chain_status, d_status, N);
    DOWN(chain_l4, d_l4, N * sizeof *l4);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
        CHECK(l4[i] == ref_l4[i], "l4 %u: %04x != %04x", i, l4[i], ref_l4[i]);
        CHECK(status[i] == chain_status[i], "status %u: %02x, the chain entry %02x", i, status[i], chain_status[i]);
        CHECK(l4[i] == chain_l4[i], "l4 %u: %04x, the chain entry %04x", i, l4[i], chain_l4[i]);
    }
    /* without the L4 array; the pool is only read */
    OUT(d_status, N, 0x55);
    CHECK(rns_rx_verify_pool_dev(d_pool, sizeof pool, LOG2, d_idx, nf, d_blk, d_len16, N, local4, local6, d_status, NULL,
                                 st) == RNS_OK, "no L4 array");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(status, d_status, N);
    CHECK(memcmp(status, ref_status, N) == 0, "without the L4 array: statuses differ");
    static uint8_t back[sizeof pool];
    DOWN(back, d_pool, sizeof pool);
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    return abi_finish("%d datagrams in %u pool buffers", N, nf);
}
