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
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rns_checksum.h"

void oracle_tx_chain_fill(uint8_t *arena, uint64_t arena_bytes, const uint64_t *frag_off, const uint32_t *frag_len,
                          const uint32_t *first, uint32_t n_frags, size_t n, uint8_t *status);

static uint64_t rng_state = 0xC0A7C4A1ull;
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
    for (uint64_t b = 0; b < bytes; b += 8) {
        const uint64_t w = next_u64();
        memcpy(arena + b, &w, bytes - b < 8 ? bytes - b : 8);
    }
    for (uint32_t i = 0; i < N; ++i) {
        uint8_t *h = arena + hoff[i];
        const uint32_t tot = (uint32_t)hl8[i] + pl16[i];
        h[0] = 0x45; h[1] = 0; h[2] = (uint8_t)(tot >> 8); h[3] = (uint8_t)tot;
        h[6] = 0x40; h[7] = 0; h[8] = 64; h[9] = proto[i];
        memcpy(h + 12, src, 4);
        memcpy(h + 16, dst, 4);                      /* both checksum fields keep their garbage */
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
    if (hipMalloc((void **)&d_arena, bytes) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed: no usable device\n");
        return 2;
    }
    HIP_OK(hipMalloc((void **)&d_status, N));
    HIP_OK(hipMalloc((void **)&d_hl8, N));
    HIP_OK(hipMalloc((void **)&d_pl16, N * sizeof *pl16));
    HIP_OK(hipMalloc((void **)&d_hblk, NB * sizeof *hblk));
    HIP_OK(hipMalloc((void **)&d_pblk, NB * sizeof *pblk));
    HIP_OK(hipStreamCreate(&st));
    HIP_OK(hipMemcpy(d_arena, arena, bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_hl8, hl8, N, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_pl16, pl16, N * sizeof *pl16, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_hblk, hblk, NB * sizeof *hblk, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_pblk, pblk, NB * sizeof *pblk, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_status, 0x55, N));
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 4, N, d_status, st) == RNS_OK,
          "rns_tx_fill_chain_packed_dev");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(back, d_arena, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status, d_status, N, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < N; ++i) {
        CHECK(ref_status[i] == (RNS_TX_IP_FILLED | RNS_TX_L4_FILLED), "oracle status %u: %02x", i, ref_status[i]);
        CHECK(status[i] == ref_status[i], "status %u: %02x != %02x", i, status[i], ref_status[i]);
    }
    uint64_t diff = 0;
    for (uint64_t b = 0; b < bytes; ++b)
        diff += back[b] != ref[b];
    CHECK(diff == 0, "%llu arena bytes differ from the oracle's", (unsigned long long)diff);
    /* without a status array, and the argument checks with a device present */
    HIP_OK(hipMemcpy(d_arena, arena, bytes, hipMemcpyHostToDevice));
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 4, N, NULL, st) == RNS_OK,
          "no status array");
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(back, d_arena, bytes, hipMemcpyDeviceToHost));
    CHECK(memcmp(back, ref, bytes) == 0, "without a status array: arena differs");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, NULL, d_pblk, d_pl16, 4, N, d_status, st) == RNS_E_INVALID,
          "NULL head lengths");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 3, N, d_status, st) == RNS_E_INVALID,
          "align 3");
    CHECK(rns_tx_fill_chain_packed_dev(d_arena, bytes, d_hblk, d_hl8, d_pblk, d_pl16, 13, N, d_status, st) == RNS_E_INVALID,
          "align 13");
    hipStreamDestroy(st);
    hipFree(d_arena); hipFree(d_status); hipFree(d_hl8); hipFree(d_pl16); hipFree(d_hblk); hipFree(d_pblk);
    free(arena); free(ref); free(back);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
