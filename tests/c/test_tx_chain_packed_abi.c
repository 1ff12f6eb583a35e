/*
 * A plain C caller of the compact-descriptor chain finalize (rns_tx_fill_chain_packed_dev), bound
 * the way the reference's Rust would bind it (extern "C" + raw pointers): no torch, no Python, the
 * HIP runtime only for device memory.  About 1000 [head, payload] chains — IPv4 with TCP, UDP and
 * ICMP heads, one in seven head-only — laid out by rns_tx_chain_packed_layout and finalized through
 * the new entry; every arena byte and status is checked against the oracle's transmit path over
 * the equivalent CSR chains (oracle/csum_oracle.c's oracle_tx_chain_fill, linked here as test
 * infrastructure only).
 *
 * Prints "all checks passed" and exits 0 on success; exits 2 when no device memory can be had.
 */
#define ABI_TEST_SEED 0xC0A7C4A1ull
#include "abi_test.h"

int main(void)
{
    enum { N = 1003, NB = (N + 63) / 64 };
    const uint8_t src[4] = {10, 0, 0, 1}, dst[4] = {10, 0, 0, 2};
    static uint8_t hl8[N], proto[N], status[N], ref_status[N];
    static uint16_t pl16[N];
    static uint64_t hblk[NB], pblk[NB], hoff[N], poff[N];
    for (uint32_t i = 0; i < N; ++i) {
        const uint64_t r = next_u64();
        proto[i] = (i % 3 == 0) ? 6 : (i % 3 == 1) ? 17 : 1;
        hl8[i] = (uint8_t)(20u + (proto[i] == 6 ? 20u : 8u));
        pl16[i] = (i % 7 == 3) ? 0 : (uint16_t)(1u + (r >> 8) % 1460u);  /* 0: a head-only datagram */
    }
    /* argument checks need no device */
    CHECK(rns_tx_fill_chain_packed_dev(NULL, 0, NULL, NULL, NULL, NULL, 4, 0, NULL, NULL) == RNS_OK, "n == 0");
    uint64_t hend = 0, pend = 0;
    CHECK(rns_tx_chain_packed_layout(hl8, pl16, N, 3, 0, 0, hblk, pblk, NULL, NULL, &hend, &pend) == RNS_E_INVALID,
          "layout align 3");
    /* heads back to back from an odd offset, payloads at 16-byte steps behind the header region */
    CHECK(rns_tx_chain_packed_layout(hl8, pl16, N, 4, 3, 0, hblk, pblk, hoff, poff, &hend, &pend) == RNS_OK,
          "layout (header region size)");
    const uint64_t pay0 = (hend + 4095) & ~4095ull;
    CHECK(rns_tx_chain_packed_layout(hl8, pl16, N, 4, 3, pay0, hblk, pblk, hoff, poff, &hend, &pend) == RNS_OK, "layout");
    CHECK(hblk[0] == 3 && pblk[0] == pay0 && hoff[64] == hblk[1] && poff[64] == pblk[1], "block offsets");
    const uint64_t bytes = pend + 16;
    uint8_t *arena = malloc(bytes), *ref = malloc(bytes), *back = malloc(bytes);
    fill_random(arena, bytes);
    for (uint32_t i = 0; i < N; ++i) {
        ipv4_fields(arena + hoff[i], (uint32_t)hl8[i] + pl16[i], proto[i], src, dst);  /* both checksum fields keep their garbage */
    }
    /* the oracle over the equivalent CSR chains */
    static uint64_t off[2 * N];
    static uint32_t len[2 * N], first[N + 1];
    uint32_t nf = 0;
    for (uint32_t i = 0; i < N; ++i) {
        first[i] = nf;
        off[nf] = hoff[i];
        len[nf++] = hl8[i];
        if (pl16[i]) {
            off[nf] = poff[i];
            len[nf++] = pl16[i];
        }
    }
    first[N] = nf;
    memcpy(ref, arena, bytes);
    oracle_tx_chain_fill(ref, bytes, off, len, first, nf, N, ref_status);

    uint8_t *d_arena = NULL, *d_status = NULL, *d_hl8 = NULL;
    uint16_t *d_pl16 = NULL;
    uint64_t *d_hblk = NULL, *d_pblk = NULL;
    hipStream_t st;
    UP(d_arena, arena, bytes);
    UP(d_hl8, hl8, N);
    UP(d_pl16, pl16, N * sizeof *pl16);
    UP(d_hblk, hblk, NB * sizeof *hblk);
    UP(d_pblk, pblk, NB * sizeof *pblk);
    OUT(d_status, N, 0x55);
    HIP_OK(abi_stream(&st));
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 4, N, d_status, st) == RNS_OK,
          "rns_tx_fill_chain_packed_dev");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(back, d_arena, bytes);
    DOWN(status, d_status, N);
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(ref_status[i] == (RNS_TX_IP_FILLED | RNS_TX_L4_FILLED), "oracle status %u: %02x", i, ref_status[i]);
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
    }
    uint64_t diff = 0;
    for (uint64_t b = 0; b < bytes; ++b)
        diff += back[b] != ref[b];
    CHECK(diff == 0, "%llu arena bytes differ from the oracle's", (unsigned long long)diff);
    /* without a status array, and the argument checks with a device present */
    UP(d_arena, arena, bytes);
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 4, N, NULL, st) == RNS_OK,
          "no status array");
    HIP_OK(hipStreamSynchronize(st));
    DOWN(back, d_arena, bytes);
    CHECK(memcmp(back, ref, bytes) == 0, "without a status array: arena differs");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, NULL, d_pblk, d_pl16, 4, N, d_status, st) == RNS_E_INVALID,
          "NULL head lengths");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 3, N, d_status, st) == RNS_E_INVALID,
          "align 3");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 13, N, d_status, st) == RNS_E_INVALID,
          "align 13");
    free(arena); free(ref); free(back);
    return abi_finish("%d chains", N);
}
