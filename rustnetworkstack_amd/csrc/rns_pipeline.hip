// The host-resident pipeline (rns_csum_batch_host), the multi-GPU contexts
// (rns_csum_batch_multi_*) and pinned host memory: the part of the C ABI
// (include/rns_checksum.h) that stages batches from host memory or fans them out over
// devices.  The device entry points are in rns_checksum.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "rns_launch.hpp"

using namespace rns;

// ---------------------------------------------------------------------------
// host-resident pipeline context
// ---------------------------------------------------------------------------
struct rns_host_ctx {
    struct Slot {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        uint8_t *d_arena = nullptr;
        uint64_t *d_off = nullptr;
        uint32_t *d_len = nullptr;
        uint16_t *d_seed = nullptr;
        uint16_t *d_out = nullptr;
        uint64_t *h_off = nullptr;  // pinned descriptor staging
        uint32_t *h_len = nullptr;
        uint16_t *h_seed = nullptr;
        uint16_t *h_out = nullptr;
        bool busy = false;
        uint32_t i0 = 0, cnt = 0;
    };
    int device = 0;
    uint64_t chunk_bytes = 0;
    uint32_t chunk_packets = 0;
    std::vector<Slot> slots;
    std::mutex mu;
};

namespace {

void free_ctx(rns_host_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    for (auto &s : c->slots) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        (void)hipFree(s.d_arena); (void)hipFree(s.d_off); (void)hipFree(s.d_len);
        (void)hipFree(s.d_seed); (void)hipFree(s.d_out);
        (void)hipHostFree(s.h_off); (void)hipHostFree(s.h_len);
        (void)hipHostFree(s.h_seed); (void)hipHostFree(s.h_out);
    }
    delete c;
}

int drain_slot(rns_host_ctx::Slot &s, uint16_t *h_out)
{
    if (!s.busy)
        return RNS_OK;
    s.busy = false;
    int st = hip_status(hipEventSynchronize(s.done));
    if (st == RNS_OK)
        std::memcpy(h_out + s.i0, s.h_out, static_cast<size_t>(s.cnt) * sizeof(uint16_t));
    return st;
}

}  // namespace

extern "C" {

int rns_host_ctx_create(int device, uint64_t chunk_bytes, uint32_t nstreams, rns_host_ctx **out)
{
    if (!out || nstreams == 0 || nstreams > 16 || chunk_bytes < 4096)
        return RNS_E_INVALID;
    *out = nullptr;
    if (int st = check_device())
        return st;
    int st = hip_status(hipSetDevice(device));
    if (st)
        return st;
    rns_host_ctx *c = new (std::nothrow) rns_host_ctx;
    if (!c)
        return RNS_E_INVALID;
    c->device = device;
    c->chunk_bytes = (chunk_bytes + 255) & ~255ull;
    c->chunk_packets = static_cast<uint32_t>(std::min<uint64_t>(c->chunk_bytes / 16, 1u << 24));
    c->slots.resize(nstreams);
    const size_t np = c->chunk_packets;
    for (auto &s : c->slots) {
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_arena), c->chunk_bytes + 256);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_off), np * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_len), np * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_seed), np * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_out), np * sizeof(uint16_t));
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.h_off), np * sizeof(uint64_t), 0);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.h_len), np * sizeof(uint32_t), 0);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.h_seed), np * sizeof(uint16_t), 0);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.h_out), np * sizeof(uint16_t), 0);
        if (e != hipSuccess) {
            free_ctx(c);
            return hip_status(e);
        }
    }
    *out = c;
    return RNS_OK;
}

int rns_host_ctx_destroy(rns_host_ctx *ctx)
{
    free_ctx(ctx);
    return RNS_OK;
}

int rns_csum_batch_host(rns_host_ctx *ctx, const uint8_t *h_arena, uint64_t arena_bytes,
                        const uint64_t *h_off, const uint32_t *h_len, const uint16_t *h_seed,
                        uint16_t *h_out, uint32_t n, uint32_t flags)
{
    if (!ctx)
        return RNS_E_INVALID;
    if (n == 0)
        return RNS_OK;
    if (!h_arena || !h_off || !h_len || !h_out)
        return RNS_E_INVALID;
    // Validate the whole batch first so a bad descriptor never reaches the device and
    // nothing is queued for a batch that cannot finish.  A chunk starts at its first
    // packet's offset rounded down to 256 bytes, so a packet fits a staging chunk iff
    // (off mod 256) + len <= chunk_bytes.
    for (uint32_t i = 0; i < n; ++i) {
        if (h_off[i] > arena_bytes || h_len[i] > arena_bytes - h_off[i])
            return RNS_E_BOUNDS;
        if (i && h_off[i] < h_off[i - 1])
            return RNS_E_ORDER;
        if ((h_off[i] & 255u) + h_len[i] > ctx->chunk_bytes)
            return RNS_E_TOOLARGE;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    int st = hip_status(hipSetDevice(ctx->device));
    if (st)
        return st;
    const size_t nslots = ctx->slots.size();
    size_t k = 0;
    uint32_t i0 = 0;
    while (i0 < n && st == RNS_OK) {
        // Chunk: packets [i0, i1) whose bytes fit one staging buffer.
        const uint64_t lo = h_off[i0] & ~255ull;  // keeps 16-byte alignment and byte parity
        uint64_t hi = lo;
        uint32_t i1 = i0;
        while (i1 < n && i1 - i0 < ctx->chunk_packets) {
            const uint64_t end = std::max(hi, h_off[i1] + h_len[i1]);
            if (end - lo > ctx->chunk_bytes)
                break;
            hi = end;
            ++i1;
        }
        if (i1 == i0) {  // (excluded by the validation pass; never leave queued slots undrained)
            st = RNS_E_TOOLARGE;
            break;
        }
        auto &s = ctx->slots[k++ % nslots];
        st = drain_slot(s, h_out);
        if (st)
            break;
        const uint32_t cnt = i1 - i0;
        std::memcpy(s.h_off, h_off + i0, cnt * sizeof(uint64_t));
        std::memcpy(s.h_len, h_len + i0, cnt * sizeof(uint32_t));
        if (h_seed)
            std::memcpy(s.h_seed, h_seed + i0, cnt * sizeof(uint16_t));
        hipError_t e = hipMemcpyAsync(s.d_arena, h_arena + lo, hi - lo, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_off, s.h_off, cnt * sizeof(uint64_t), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_len, s.h_len, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && h_seed)
            e = hipMemcpyAsync(s.d_seed, s.h_seed, cnt * sizeof(uint16_t), hipMemcpyHostToDevice, s.stream);
        if (e != hipSuccess) {
            st = hip_status(e);
            break;
        }
        // Offsets stay absolute: the kernel sees arena = staging - lo (never dereferenced below staging).
        CsumArgs a{};
        a.arena = s.d_arena - lo;
        a.arena_bytes = hi;
        a.base_adjust = 0;
        a.off = s.d_off;
        a.len = s.d_len;
        a.seed = h_seed ? s.d_seed : nullptr;
        a.out = s.d_out;
        a.n = cnt;
        a.flags = flags;
        const Shape sh = pick_shape(static_cast<uint32_t>(std::min<uint64_t>((hi - lo) / cnt, 1u << 30)));
        st = dispatch<false>(a, sh.variant, sh.G, sh.U, sh.max_blocks, s.stream);
        if (st)
            break;
        e = hipMemcpyAsync(s.h_out, s.d_out, cnt * sizeof(uint16_t), hipMemcpyDeviceToHost, s.stream);
        if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
        if (e != hipSuccess) {
            st = hip_status(e);
            break;
        }
        s.busy = true;
        s.i0 = i0;
        s.cnt = cnt;
        i0 = i1;
    }
    for (auto &s : ctx->slots) {
        int d = drain_slot(s, h_out);
        if (st == RNS_OK)
            st = d;
    }
    return st;
}

// ---------------------------------------------------------------------------
// Multi-GPU batches: packets are independent, so a batch
// is cut into contiguous packet ranges of about equal BYTES, one per GPU; each GPU
// checksums its range from its own HBM (device-resident) or through its own
// staging context and PCIe link (host-resident).  No bytes cross xGMI and no
// collective is needed: each range's results land in their slice of h_out.
// ---------------------------------------------------------------------------
struct rns_multi_ctx {
    std::vector<rns_host_ctx *> ctx;
};

int rns_multi_ctx_create(const int *devices, uint32_t ndev, uint64_t chunk_bytes, uint32_t nstreams,
                         rns_multi_ctx **out)
{
    if (!out || !devices || ndev == 0 || ndev > 64)
        return RNS_E_INVALID;
    *out = nullptr;
    rns_multi_ctx *m = new (std::nothrow) rns_multi_ctx;
    if (!m)
        return RNS_E_INVALID;
    for (uint32_t i = 0; i < ndev; ++i) {
        rns_host_ctx *c = nullptr;
        const int st = rns_host_ctx_create(devices[i], chunk_bytes, nstreams, &c);
        if (st) {
            rns_multi_ctx_destroy(m);
            return st;
        }
        m->ctx.push_back(c);
    }
    *out = m;
    return RNS_OK;
}

int rns_multi_ctx_destroy(rns_multi_ctx *ctx)
{
    if (ctx) {
        for (rns_host_ctx *c : ctx->ctx)
            rns_host_ctx_destroy(c);
        delete ctx;
    }
    return RNS_OK;
}

extern "C++" {
namespace {
// Cut [0, n) into `parts` contiguous ranges of about equal byte totals: bounds[0..parts].
std::vector<uint32_t> split_by_bytes(const uint32_t *len, uint32_t n, uint32_t parts)
{
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i)
        total += len[i];
    std::vector<uint32_t> bounds(parts + 1, n);
    bounds[0] = 0;
    uint64_t acc = 0;
    uint32_t i = 0;
    for (uint32_t k = 1; k < parts; ++k) {
        const uint64_t target = total * k / parts;
        while (i < n && acc + len[i] <= target)
            acc += len[i++];
        bounds[k] = std::max(i, bounds[k - 1]);
    }
    return bounds;
}
}  // namespace
}  // extern "C++"

int rns_csum_batch_multi_host(rns_multi_ctx *ctx, const uint8_t *h_arena, uint64_t arena_bytes,
                              const uint64_t *h_off, const uint32_t *h_len, const uint16_t *h_seed,
                              uint16_t *h_out, uint32_t n, uint32_t flags)
{
    if (!ctx || ctx->ctx.empty())
        return RNS_E_INVALID;
    if (n == 0)
        return RNS_OK;
    if (!h_arena || !h_off || !h_len || !h_out)
        return RNS_E_INVALID;
    const uint32_t parts = static_cast<uint32_t>(ctx->ctx.size());
    const std::vector<uint32_t> b = split_by_bytes(h_len, n, parts);
    std::vector<int> st(parts, RNS_OK);
    auto run = [&](uint32_t k) {
        const uint32_t i0 = b[k], cnt = b[k + 1] - b[k];
        if (cnt)
            st[k] = rns_csum_batch_host(ctx->ctx[k], h_arena, arena_bytes, h_off + i0, h_len + i0,
                                        h_seed ? h_seed + i0 : nullptr, h_out + i0, cnt, flags);
    };
    std::vector<std::thread> workers;
    for (uint32_t k = 1; k < parts; ++k) {
        try {
            workers.emplace_back(run, k);
        } catch (...) {
            run(k);  // no thread available: run this range inline
        }
    }
    run(0);
    for (auto &w : workers)
        w.join();
    for (int x : st)
        if (x)
            return x;
    return RNS_OK;
}

int rns_csum_batch_multi_dev(const rns_dev_batch *batches, uint32_t nbatches, uint32_t flags)
{
    if (nbatches == 0)
        return RNS_OK;
    if (!batches)
        return RNS_E_INVALID;
    if (int st = check_device())
        return st;
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess)
        return RNS_E_NODEVICE;
    int st = RNS_OK;
    for (uint32_t k = 0; k < nbatches && st == RNS_OK; ++k) {  // launches are asynchronous: GPUs run together
        const rns_dev_batch &d = batches[k];
        st = hip_status(hipSetDevice(d.device));
        if (st == RNS_OK)
            st = rns_csum_batch_dev(d.d_arena, d.arena_bytes, d.d_off, d.d_len, d.d_seed, d.d_out, d.n, flags,
                                    d.len_hint, d.d_bad, d.stream);
    }
    (void)hipSetDevice(prev);
    return st;
}

int rns_host_alloc(uint64_t bytes, void **out)
{
    if (!out)
        return RNS_E_INVALID;
    *out = nullptr;
    if (int st = check_device())
        return st;
    return hip_status(hipHostMalloc(out, bytes, 0));
}

int rns_host_free(void *p) { return hip_status(hipHostFree(p)); }

}  // extern "C"
