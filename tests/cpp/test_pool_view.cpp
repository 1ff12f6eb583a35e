// The plain-C++ header decode of the pool receive view (csrc/rns_k_pool_view.hpp) on the host: the IP
// header length, the family and the protocol against IPv4 and IPv6 heads built by hand, byte by byte, and
// the port swaps against ports whose four bytes all differ.
#include <cstdio>
#include <cstring>

#include "rns_k_pool_view.hpp"

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

// The head's bytes as the dwords a lane reads (the buffers are 4-byte aligned; memcpy keeps the host's
// sanitizers content whatever the array's alignment).
static void as_dwords(const uint8_t *b, uint32_t *w, int n) { std::memcpy(w, b, 4 * n); }

int main()
{
    const uint32_t protos[4] = {1, 6, 17, 58};
    // IPv4: every header length the IHL field names from 5 to 15, the bytes around the fields read all set
    for (uint32_t ihl = 5; ihl <= 15; ++ihl) {
        for (uint32_t proto : protos) {
            uint8_t b[64];
            std::memset(b, 0xff, sizeof(b));
            b[0] = static_cast<uint8_t>(0x40 | ihl);
            b[9] = static_cast<uint8_t>(proto);
            uint32_t w[16];
            as_dwords(b, w, 16);
            const IpHead d = ip_head(w);
            CHECK(!d.v6 && d.ip_hdr == 4 * ihl && d.proto == proto, "IPv4 ihl %u proto %u: v6 %d ip_hdr %u proto %u", ihl, proto,
                  d.v6, d.ip_hdr, d.proto);
        }
    }
    // IPv6: 40 bytes whatever the low nibble of the first byte (a traffic-class bit), next header at byte 6
    for (uint32_t low = 0; low < 16; low += 5) {
        for (uint32_t proto : protos) {
            uint8_t b[64];
            std::memset(b, 0xff, sizeof(b));
            b[0] = static_cast<uint8_t>(0x60 | low);
            b[6] = static_cast<uint8_t>(proto);
            b[9] = static_cast<uint8_t>(proto ^ 0x55);  // IPv4's protocol byte: part of the source address here
            uint32_t w[16];
            as_dwords(b, w, 16);
            const IpHead d = ip_head(w);
            CHECK(d.v6 && d.ip_hdr == 40 && d.proto == proto, "IPv6 low %u proto %u: v6 %d ip_hdr %u proto %u", low, proto, d.v6,
                  d.ip_hdr, d.proto);
        }
    }
    // the ports: four distinct bytes, and the extremes
    const uint8_t ports[3][4] = {{0x12, 0x34, 0xab, 0xcd}, {0x00, 0x01, 0xff, 0xfe}, {0x80, 0x00, 0x00, 0x80}};
    for (const auto &p : ports) {
        uint32_t t0;
        as_dwords(p, &t0, 1);
        const uint32_t sport = (static_cast<uint32_t>(p[0]) << 8) | p[1], dport = (static_cast<uint32_t>(p[2]) << 8) | p[3];
        CHECK(l4_sport(t0) == sport && l4_dport(t0) == dport, "ports %04x %04x: got %04x %04x", sport, dport, l4_sport(t0),
              l4_dport(t0));
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
