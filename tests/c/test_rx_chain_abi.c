/*
 * A plain C caller of the receive verify over fragment chains (rns_rx_verify_chain_dev), bound the
 * way the reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the HIP
 * runtime only for device memory.  60 datagrams — IPv4 TCP, IPv6 TCP and IPv4 ICMP, every fifth
 * with a flipped byte — lie in shuffled pool buffers as recv_packet leaves them (512-byte
 * fragments, netif.rs:65-83) or cut at odd places; every status and L4 value is checked against the
 * receive path restated here over the oracle's primitives (oracle/csum_oracle.c, linked as test
 * infrastructure only): header checksum over the first fragment, trim_head, the pseudo-header
 * with the chain's length, compute_buffer_ones_comp over the trimmed fragments.
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0x5C4A1Full
#include "abi_test.h"

enum { N = 60, BUF = 512, MAXLEN = 2048, MAXFR = 8, NBUF = N * MAXFR };

static const uint8_t local4[4] = {10, 0, 0, 2}, remote4[4] = {10, 0, 0, 1};
static const uint8_t local6[16] = {0xfd, [15] = 2}, remote6[16] = {0xfd, [15] = 1};
static const rx_addrs addrs = {remote4, local4, remote6, local6};

int main(void)
{
    static uint8_t pool[NBUF * BUF + 16], dgram[MAXFR * BUF], status[N], ref_status[N];
    static uint16_t l4[N], ref_l4[N];
    static uint64_t off[NBUF];
    static uint32_t len[NBUF], first[N + 1], order[NBUF];
    shuffled_order(order, NBUF);
    memset(pool, 0xEE, sizeof pool);
    uint32_t nf = 0;
    int accepted = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const int k = (int)(i % 3);
        const uint32_t hdr = k == 1 ? 40 : 20;
        /* fragment lengths first: i even, a datagram cut into full buffers as recv_packet leaves it;
         * i odd, cut at odd places (the first fragment holds the header and 1 or 3 bytes more) */
        uint32_t fl[MAXFR], nfr = 0, dl = 0;
        if (i & 1) {
            nfr = 2 + (uint32_t)(next_u64() % (MAXFR - 1));
            fl[0] = hdr + 1 + (i & 2);
            fl[1] = 20 + (uint32_t)(next_u64() % (BUF - 22));
            for (uint32_t f = 2; f < nfr; ++f)
                fl[f] = 1 + (uint32_t)(next_u64() % (BUF - 2));
            for (uint32_t f = 0; f < nfr; ++f)
                dl += fl[f];
        } else {
            dl = hdr + 20 + (uint32_t)(next_u64() % (MAXLEN - hdr - 20 + 1));
            for (uint32_t pos = 0; pos < dl; pos += BUF)
                fl[nfr++] = dl - pos < BUF ? dl - pos : BUF;
        }
        make_datagram(dgram, dl, k, &addrs);
        if (i % 5 == 4)
            dgram[hdr + (next_u64() % (dl - hdr))] ^= 0x10;
        first[i] = nf;
        const uint8_t *fbase[MAXFR];
        size_t flen[MAXFR];
        for (uint32_t f = 0, pos = 0; f < nfr; pos += fl[f++]) {
            off[nf] = (uint64_t)order[nf] * BUF + ((i & 1) ? (uint32_t)(next_u64() % 3) : 0);  /* odd: <= BUF - 2 bytes */
            len[nf] = fl[f];
            fbase[f] = memcpy(pool + off[nf], dgram + pos, fl[f]);
            flen[f] = fl[f];
            ++nf;
        }
        rx_reference(fbase, flen, nfr, local4, local6, &ref_status[i], &ref_l4[i]);
        accepted += (ref_status[i] & RNS_RX_ACCEPT) != 0;
    }
    first[N] = nf;
    /* the intact full-buffer chains verify; a chain cut at odd places folds differently (util.rs:97-99) */
    CHECK(accepted >= N / 3 && accepted <= N / 2, "the oracle accepts %d of %d", accepted, N);

    /* argument checks need no device */
    CHECK(rns_rx_verify_chain_dev(NULL, 0, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL) == RNS_OK, "n == 0");
    CHECK(rns_rx_verify_chain_dev(pool, sizeof pool, off, len, nf, first, N, local4, local6, NULL, NULL, NULL) ==
              RNS_E_INVALID, "NULL status");
    CHECK(rns_rx_verify_chain_dev(pool, sizeof pool, NULL, len, nf, first, N, local4, local6, status, NULL, NULL) ==
              RNS_E_INVALID, "NULL offsets");

    uint8_t *d_pool = NULL, *d_status = NULL;
    uint16_t *d_l4 = NULL;
    uint64_t *d_off = NULL;
    uint32_t *d_len = NULL, *d_first = NULL;
    hipStream_t st;
    UP(d_pool, pool, sizeof pool);
    UP(d_off, off, NBUF * sizeof *off);
    UP(d_len, len, NBUF * sizeof *len);
    UP(d_first, first, (N + 1) * sizeof *first);
    OUT(d_status, N, 0x55);
    OUT(d_l4, N * sizeof *l4, 0);
    HIP_OK(abi_stream(&st));
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, d_l4, st) ==
              RNS_OK, "rns_rx_verify_chain_dev");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(status, d_status, N);
    DOWN(l4, d_l4, N * sizeof *l4);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
        CHECK(l4[i] == ref_l4[i], "l4 %u: %04x != %04x", i, l4[i], ref_l4[i]);
    }
    /* without the L4 array; the pool is only read */
    OUT(d_status, N, 0x55);
    CHECK(rns_rx_verify_chain_dev(d_pool, sizeof pool, d_off, d_len, nf, d_first, N, local4, local6, d_status, NULL, st) ==
              RNS_OK, "no L4 array");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(status, d_status, N);
    CHECK(memcmp(status, ref_status, N) == 0, "without the L4 array: statuses differ");
    static uint8_t back[sizeof pool];
    DOWN(back, d_pool, sizeof pool);
    CHECK(memcmp(back, pool, sizeof pool) == 0, "the pool changed");
    return abi_finish("%d datagrams in %u fragments", N, nf);
}
