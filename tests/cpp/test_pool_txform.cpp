// The plain-C++ parts of the pool transmit form (csrc/rns_k_pool_txform.hpp) on the host: the IPv4 and IPv6
// head words against headers written byte by byte (the IPv4 checksum recomputed over the bytes), the build
// workspace's size against the three formulas it replaced, and the status bits the builders share.
#include <cstdio>
#include <cstring>

#include "rns_k_pool_txform.hpp"

using namespace rns;

static int g_fail = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++g_fail <= 20) {                             \
                std::fprintf(stderr, "line %d: ", __LINE__);  \
                std::fprintf(stderr, __VA_ARGS__);            \
                std::fprintf(stderr, "\n");                   \
            }                                                 \
        }                                                     \
    } while (0)

// RFC 1071 over n bytes (n even), big-endian words, folded.
static uint32_t sum_be(const uint8_t *b, int n)
{
    uint32_t s = 0;
    for (int k = 0; k < n; k += 2)
        s += (static_cast<uint32_t>(b[k]) << 8) | b[k + 1];
    while (s > 0xffff)
        s = (s & 0xffff) + (s >> 16);
    return s;
}

// The workspace formulas as rns_k_args.hpp had them (the listen one with its table's slots restated).
static uint64_t blocks(uint64_t n) { return (n + 255) / 256; }
static uint64_t old_echo(uint64_t n) { return 16ull * (blocks(n) + 1) + 4ull * n; }
static uint64_t old_udp_tx(uint64_t n) { return 16ull * (blocks(n) + 1) + 4ull * n; }
static uint64_t slots(uint64_t n)
{
    uint64_t s = 64;
    while (s < 2 * n)
        s <<= 1;
    return s;
}
static uint64_t old_listen(uint64_t n) { return 16ull * (blocks(n) + 1) + 12ull * slots(n) + 4ull * n; }

int main()
{
    const uint8_t l4[4] = {192, 168, 7, 1}, p4[4] = {10, 0xff, 0, 0xfe};
    uint8_t l6[16], p6[16];
    for (int k = 0; k < 16; ++k) {
        l6[k] = static_cast<uint8_t>(0x20 + 7 * k);
        p6[k] = static_cast<uint8_t>(0xff - 13 * k);
    }
    LocalAddrs local;
    set_local(local, l4, l6);
    uint32_t peer4, peer6[4];
    std::memcpy(&peer4, p4, 4);
    std::memcpy(peer6, p6, 16);
    CHECK(std::memcmp(&local.v4, l4, 4) == 0 && std::memcmp(local.v6, l6, 16) == 0, "set_local");

    // IPv4: the ids' ends, and totals that wrap as u16 (24 + 65535 - 24, 28 + 65535)
    const uint32_t ids[4] = {0, 0xffff, 0x1234, 0xff00}, totals[5] = {24, 28, 1500, 65535, 28 + 65535}, protos[2] = {1, 17};
    for (uint32_t id : ids) {
        for (uint32_t total : totals) {
            for (uint32_t proto : protos) {
                uint8_t b[20] = {0x45, 0, static_cast<uint8_t>(total >> 8), static_cast<uint8_t>(total), static_cast<uint8_t>(id >> 8),
                                 static_cast<uint8_t>(id), 0, 0, 64, static_cast<uint8_t>(proto), 0, 0};
                std::memcpy(b + 12, l4, 4);
                std::memcpy(b + 16, p4, 4);
                const uint32_t ck = sum_be(b, 20) ^ 0xffffu;
                b[10] = static_cast<uint8_t>(ck >> 8);
                b[11] = static_cast<uint8_t>(ck);
                const Ip4Head h = ip4_head(total, id, proto, local.v4, peer4);
                CHECK(std::memcmp(h.d, b, 20) == 0, "ip4_head total %u id %u proto %u", total, id, proto);
                uint8_t got[20];
                std::memcpy(got, h.d, 20);
                CHECK(sum_be(got, 20) == 0xffffu, "ip4_head's checksum, total %u id %u proto %u", total, id, proto);
            }
        }
    }
    CHECK(addr_sum4(local.v4, peer4) == ((192u << 8) + 168 + (7u << 8) + 1 + (10u << 8) + 0xff + 0xfe), "addr_sum4");

    // IPv6: payload lengths up to the u16's end, the two next headers
    const uint32_t plens[4] = {4, 8, 1480, 65535}, nexts[2] = {58, 17};
    for (uint32_t plen : plens) {
        for (uint32_t next : nexts) {
            uint8_t b[40] = {0x60, 0, 0, 0, static_cast<uint8_t>(plen >> 8), static_cast<uint8_t>(plen), static_cast<uint8_t>(next), 64};
            std::memcpy(b + 8, l6, 16);
            std::memcpy(b + 24, p6, 16);
            const Ip6Head h = ip6_head(plen, next, local.v6, peer6);
            CHECK(std::memcmp(h.d, b, 40) == 0, "ip6_head plen %u next %u", plen, next);
        }
    }
    uint32_t s6 = 0;
    for (int k = 0; k < 16; k += 2)
        s6 += (static_cast<uint32_t>(l6[k]) << 8) + l6[k + 1] + (static_cast<uint32_t>(p6[k]) << 8) + p6[k + 1];
    CHECK(addr_sum6(local.v6, peer6) == s6, "addr_sum6 %u, by hand %u", addr_sum6(local.v6, peer6), s6);

    // the workspace
    const uint64_t ns[6] = {0, 1, 255, 256, 257, 65537};
    for (uint64_t n : ns) {
        const uint64_t got = build_work_bytes(n);
        CHECK(got == old_echo(n) && got == old_udp_tx(n) && got + 12 * slots(n) == old_listen(n) && got % 8 == 4 * (n & 1),
              "build_work_bytes(%llu) = %llu", static_cast<unsigned long long>(n), static_cast<unsigned long long>(got));
    }

    // the status bits: one set for both builders
    static_assert(RNS_ECHO_REQUEST == 0x01 && RNS_ECHO_BUILT == 0x02 && RNS_ECHO_NOBUF == 0x04 && RNS_ECHO_BADBUF == 0x08, "echo bits");
    static_assert(RNS_UDPTX_SEND == 0x01 && RNS_UDPTX_BUILT == 0x02 && RNS_UDPTX_NOBUF == 0x04 && RNS_UDPTX_BADBUF == 0x08, "send bits");
    CHECK(kTxItem == RNS_UDPTX_SEND && kTxBuilt == RNS_UDPTX_BUILT && kTxNobuf == RNS_UDPTX_NOBUF && kTxBadbuf == RNS_UDPTX_BADBUF,
          "the shared status bits");

    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
