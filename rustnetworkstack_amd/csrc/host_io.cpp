// Batched datagram I/O for the receive / transmit ends of the checksum path
// (SURVEY §8f row 3).  The reference moves one packet per call: recv_packet
// (netif.rs:65-83) readv()s one datagram from the TUN fd into a 2048-byte MRU
// NetBuffer (tun.c:84-86), send_packet (netif.rs:85-98) writev()s one (tun.c:88-90).
// These entry points move a whole batch between such an fd (TUN, or any datagram
// fd: SOCK_SEQPACKET / SOCK_DGRAM) and an arena, so the batch can go to the GPU in
// one copy (rns_rx_verify_packed_dev / rns_rx_verify_dev / rns_tx_fill_packed_dev).
// On a socket fd a batch takes recvmmsg / sendmmsg: up to kMmsg datagrams per system
// call; a TUN fd moves one datagram per read / writev (its driver has no batched call).
// rns_io_send_batch_chain sends NetBuffer chains as send_packet does — each datagram's
// fragments as one gather write (to_iovec + tun_send's writev, netif.rs:51-63, 85-98).
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <unistd.h>

#include "rns_checksum.h"

namespace {

constexpr unsigned kMmsg = 64;  // datagrams per recvmmsg / sendmmsg call
constexpr uint32_t kChainIov = RNS_IO_MAX_FRAGS;  // fragments per datagram (netif.rs:22 MAX_VECS)

// Waits up to timeout_ms for the first datagram; 1 = readable, 0 = timeout, < 0 = error.
int wait_first(int fd, int timeout_ms)
{
    struct pollfd pfd = {fd, POLLIN, 0};
    int pr;
    do {
        pr = poll(&pfd, 1, timeout_ms);  // wait for the first datagram only
    } while (pr < 0 && errno == EINTR);
    return pr < 0 ? RNS_E_IO : pr;
}

// The fd in non-blocking mode for the duration of one batch (TUN reads), restored after.
struct NonBlocking {
    int fd, flags = -1;
    bool changed = false;
    explicit NonBlocking(int f) : fd(f)
    {
        flags = fcntl(fd, F_GETFL);
        if (flags >= 0 && !(flags & O_NONBLOCK))
            changed = fcntl(fd, F_SETFL, flags | O_NONBLOCK) == 0;
    }
    bool ok() const { return flags >= 0 && ((flags & O_NONBLOCK) || changed); }
    ~NonBlocking()
    {
        if (changed)
            (void)fcntl(fd, F_SETFL, flags);
    }
};

// One recvmmsg round into k buffers of cap bytes at bufs[i]: the number of messages
// (their lengths in len[], each flagged in trunc[] if it did not fit), 0 when nothing
// is queued, RNS_E_IO on an error, -ENOTSOCK when the fd is not a socket.
int recv_round(int fd, uint8_t *const *bufs, uint64_t cap, unsigned k, uint32_t *len, bool *trunc)
{
    struct mmsghdr mh[kMmsg];
    struct iovec iov[kMmsg];
    std::memset(mh, 0, sizeof(mh));
    for (unsigned i = 0; i < k; ++i) {
        iov[i].iov_base = bufs[i];
        iov[i].iov_len = cap;
        mh[i].msg_hdr.msg_iov = &iov[i];
        mh[i].msg_hdr.msg_iovlen = 1;
    }
    int r;
    do {
        r = recvmmsg(fd, mh, k, MSG_DONTWAIT | MSG_TRUNC, nullptr);
    } while (r < 0 && errno == EINTR);
    if (r < 0) {
        if (errno == ENOTSOCK)
            return -ENOTSOCK;
        return (errno == EAGAIN || errno == EWOULDBLOCK) ? 0 : RNS_E_IO;
    }
    for (int i = 0; i < r; ++i) {
        len[i] = mh[i].msg_len;
        trunc[i] = (mh[i].msg_hdr.msg_flags & MSG_TRUNC) || mh[i].msg_len > cap;
    }
    return r;
}

// The receive loop of rns_io_recv_batch_chain and rns_io_recv_batch_pool (rns_checksum.h describes
// it there): datagrams into the next free buffers, h_free permuted so that its first *n_frags_out
// entries are the buffers in use, in fragment order.  `out` records the descriptors of its form:
// begin() once the arguments are valid; frag(j, buf, len) for fragment j = buffer `buf` holding len
// bytes; datagram(i, first, cnt, len) for datagram i = fragments [first, first + cnt), len bytes.
template <class Out>
int recv_chain_loop(int fd, uint8_t *h_pool, uint32_t buf_bytes, uint32_t *h_free, uint32_t n_free, uint32_t mru,
                    uint32_t max_pkts, uint32_t *n_frags_out, int timeout_ms, Out out)
{
    if (fd < 0 || !h_pool || !h_free || !n_frags_out || buf_bytes == 0 || mru == 0 || max_pkts == 0)
        return RNS_E_INVALID;
    // new_prealloc(mru): the buffers a datagram is offered, the last one cut so they hold mru bytes
    const uint64_t need64 = (static_cast<uint64_t>(mru) + buf_bytes - 1) / buf_bytes;
    if (need64 > kChainIov)
        return RNS_E_INVALID;
    const uint32_t need = static_cast<uint32_t>(need64);
    const uint32_t last_cap = mru - (need - 1) * buf_bytes;  // 1..buf_bytes
    if (max_pkts > static_cast<uint32_t>(INT_MAX))
        max_pkts = static_cast<uint32_t>(INT_MAX);
    *n_frags_out = 0;
    out.begin();
    if (n_free < need)
        return 0;
    const int pr = wait_first(fd, timeout_ms);
    if (pr <= 0)
        return pr;
    uint32_t n = 0, used = 0;  // datagrams kept; h_free[0..used) in use, in fragment order
    int status = 0;
    // trim_tail: datagram n of len bytes lies in the buffers h_free[at..at + need).  It keeps the
    // ceil(len / buf_bytes) it filled; they move to h_free[used..] (used <= at: the swaps run
    // upwards, so every source entry is still in place when it is read) and the rest stay free.
    auto keep = [&](uint32_t at, uint32_t len) {
        const uint32_t cnt = (len + buf_bytes - 1) / buf_bytes;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t b = h_free[at + j];
            h_free[at + j] = h_free[used + j];
            h_free[used + j] = b;
            out.frag(used + j, b, j + 1 < cnt ? buf_bytes : len - j * buf_bytes);
        }
        out.datagram(n++, used, cnt, len);
        used += cnt;
    };
    auto fill_iov = [&](struct iovec *v, uint32_t at) {
        for (uint32_t j = 0; j < need; ++j) {
            v[j].iov_base = h_pool + static_cast<uint64_t>(h_free[at + j]) * buf_bytes;
            v[j].iov_len = j + 1 < need ? buf_bytes : last_cap;
        }
    };
    bool sock = true;
    while (sock && n < max_pkts) {  // sockets: recvmmsg, each message one datagram's buffers
        unsigned k = max_pkts - n < kMmsg ? max_pkts - n : kMmsg;
        if ((n_free - used) / need < k)
            k = (n_free - used) / need;
        if (k == 0)
            break;
        struct mmsghdr mh[kMmsg];
        struct iovec iov[kMmsg * kChainIov];
        std::memset(mh, 0, sizeof(mh));
        const uint32_t at0 = used;
        for (unsigned i = 0; i < k; ++i) {
            fill_iov(iov + i * kChainIov, at0 + i * need);
            mh[i].msg_hdr.msg_iov = iov + i * kChainIov;
            mh[i].msg_hdr.msg_iovlen = need;
        }
        int r;
        do {
            r = recvmmsg(fd, mh, k, MSG_DONTWAIT | MSG_TRUNC, nullptr);
        } while (r < 0 && errno == EINTR);
        if (r < 0) {
            if (errno == ENOTSOCK) {
                sock = false;
                break;
            }
            if (errno != EAGAIN && errno != EWOULDBLOCK)
                status = RNS_E_IO;
            break;
        }
        bool any = false;
        for (int i = 0; i < r; ++i) {
            const uint32_t len = mh[i].msg_len;
            if (len == 0)  // an empty datagram: skipped, those after it are kept
                continue;
            any = true;
            if ((mh[i].msg_hdr.msg_flags & MSG_TRUNC) || len > mru)  // longer than mru: dropped, takes no buffer
                continue;
            keep(at0 + static_cast<uint32_t>(i) * need, len);
        }
        // the queue is drained; a round of nothing but empty reads also ends the call (a closed
        // stream peer reads as empty datagrams for ever)
        if (static_cast<unsigned>(r) < k || !any)
            break;
    }
    if (!sock) {
        NonBlocking nb(fd);  // a TUN fd: one readv per datagram, like tun_recv
        if (!nb.ok())
            return RNS_E_IO;
        uint8_t spill;  // the byte past mru: a longer datagram shows as mru + 1
        while (n < max_pkts && n_free - used >= need) {
            struct iovec v[kChainIov + 1];
            fill_iov(v, used);
            v[need].iov_base = &spill;
            v[need].iov_len = 1;
            const ssize_t r = readv(fd, v, static_cast<int>(need + 1));
            if (r < 0) {
                if (errno == EINTR)
                    continue;
                if (errno != EAGAIN && errno != EWOULDBLOCK)
                    status = RNS_E_IO;
                break;
            }
            if (r == 0)
                break;
            if (static_cast<uint64_t>(r) > mru)
                continue;
            keep(used, static_cast<uint32_t>(r));
        }
    }
    *n_frags_out = used;
    return (n == 0 && status) ? status : static_cast<int>(n);
}

// The send loop rns_io_send_batch_chain and rns_io_send_batch_pool share: frags(i, v) writes datagram
// i's fragments (1..kChainIov, checked by the caller) into v and returns their number.  Sockets:
// sendmmsg, each message one datagram's fragments; a TUN fd: one writev per datagram, like tun_send.
template <class Frags>
int send_chain_loop(int fd, uint32_t n_pkts, Frags frags)
{
    uint32_t i = 0;
    bool sock = true;
    while (sock && i < n_pkts) {
        const unsigned k = n_pkts - i < kMmsg ? n_pkts - i : kMmsg;
        struct mmsghdr mh[kMmsg];
        struct iovec iov[kMmsg * kChainIov];
        std::memset(mh, 0, sizeof(mh));
        for (unsigned j = 0; j < k; ++j) {
            struct iovec *v = iov + j * kChainIov;
            mh[j].msg_hdr.msg_iovlen = frags(i + j, v);
            mh[j].msg_hdr.msg_iov = v;
        }
        int w;
        do {
            w = sendmmsg(fd, mh, k, 0);
        } while (w < 0 && errno == EINTR);
        if (w < 0) {
            if (errno == ENOTSOCK && i == 0) {
                sock = false;
                break;
            }
            return i ? static_cast<int>(i) : RNS_E_IO;
        }
        i += static_cast<uint32_t>(w);
    }
    for (; i < n_pkts; ++i) {
        struct iovec v[kChainIov];
        const uint32_t nf = frags(i, v);
        ssize_t w;
        do {
            w = writev(fd, v, static_cast<int>(nf));
        } while (w < 0 && errno == EINTR);
        if (w < 0)
            return i ? static_cast<int>(i) : RNS_E_IO;
    }
    return static_cast<int>(n_pkts);
}

}  // namespace

extern "C" {

int rns_io_recv_batch(int fd, uint8_t *h_arena, uint64_t slot_bytes, uint32_t max_pkts, uint64_t *h_off,
                      uint32_t *h_len, int timeout_ms)
{
    if (fd < 0 || !h_arena || !h_off || !h_len || slot_bytes == 0 || max_pkts == 0)
        return RNS_E_INVALID;
    if (max_pkts > static_cast<uint32_t>(INT_MAX))  // the count is returned as an int
        max_pkts = static_cast<uint32_t>(INT_MAX);
    const int pr = wait_first(fd, timeout_ms);
    if (pr <= 0)
        return pr;
    uint32_t n = 0;
    int status = 0;
    bool sock = true;
    while (sock && n < max_pkts) {  // sockets: recvmmsg straight into the next slots
        const unsigned k = max_pkts - n < kMmsg ? max_pkts - n : kMmsg;
        uint8_t *bufs[kMmsg];
        for (unsigned i = 0; i < k; ++i)
            bufs[i] = h_arena + static_cast<uint64_t>(n + i) * slot_bytes;
        uint32_t len[kMmsg];
        bool trunc[kMmsg];
        const int r = recv_round(fd, bufs, slot_bytes, k, len, trunc);
        if (r == -ENOTSOCK) {
            sock = false;
            break;
        }
        if (r < 0)
            status = r;
        if (r <= 0)
            return (n == 0 && status) ? status : static_cast<int>(n);
        int eof = 0;
        uint32_t kept = 0;
        for (int i = 0; i < r; ++i) {
            if (len[i] == 0) {  // peer closed (a zero-length datagram cannot be told from it)
                eof = 1;
                break;
            }
            if (trunc[i])  // longer than its slot: dropped, never handed on truncated
                continue;
            const uint32_t d = n + kept;
            if (d != n + static_cast<uint32_t>(i))  // close the gap a dropped datagram left
                std::memmove(h_arena + static_cast<uint64_t>(d) * slot_bytes, bufs[i], len[i]);
            h_off[d] = static_cast<uint64_t>(d) * slot_bytes;
            h_len[d] = len[i];
            ++kept;
        }
        n += kept;
        if (eof || static_cast<unsigned>(r) < k)
            return static_cast<int>(n);
    }
    if (sock)
        return static_cast<int>(n);
    NonBlocking nb(fd);  // a TUN fd: one datagram per read, like tun_recv
    if (!nb.ok())
        return RNS_E_IO;
    while (n < max_pkts) {
        uint8_t *slot = h_arena + static_cast<uint64_t>(n) * slot_bytes;
        const ssize_t r = read(fd, slot, slot_bytes);
        if (r < 0) {
            if (errno == EINTR)
                continue;
            if (errno != EAGAIN && errno != EWOULDBLOCK)
                status = RNS_E_IO;
            break;
        }
        if (r == 0)
            break;
        if (static_cast<uint64_t>(r) > slot_bytes)
            continue;
        h_off[n] = static_cast<uint64_t>(n) * slot_bytes;
        h_len[n] = static_cast<uint32_t>(r);
        ++n;
    }
    return (n == 0 && status) ? status : static_cast<int>(n);
}

int rns_io_recv_batch_packed(int fd, uint8_t *h_arena, uint64_t arena_bytes, uint32_t mru, uint32_t max_pkts,
                             uint16_t *h_len16, uint64_t *h_blk_off, uint64_t *h_end, int timeout_ms)
{
    if (fd < 0 || !h_arena || !h_len16 || !h_blk_off || !h_end || mru == 0 || mru > 0xFFFFu || max_pkts == 0)
        return RNS_E_INVALID;
    if (max_pkts > static_cast<uint32_t>(INT_MAX))
        max_pkts = static_cast<uint32_t>(INT_MAX);
    *h_end = 0;
    const int pr = wait_first(fd, timeout_ms);
    if (pr <= 0)
        return pr;
    const uint64_t step = (static_cast<uint64_t>(mru) + 15) & ~15ull;  // >= any padded datagram
    uint64_t pos = 0;  // where the next datagram goes (16-byte aligned)
    uint32_t n = 0;
    int status = 0;
    auto take = [&](uint32_t len) {  // datagram n of len bytes now lies at pos
        if ((n & 63u) == 0)
            h_blk_off[n >> 6] = pos;
        h_len16[n] = static_cast<uint16_t>(len);
        ++n;
        pos = (pos + len + 15) & ~15ull;
    };
    bool sock = true;
    while (sock && n < max_pkts) {
        // recvmmsg into MRU-sized buffers (16-byte steps) from pos on, then each datagram moves
        // down to its packed place (at or below its buffer: one memmove of its own bytes)
        const uint64_t room = arena_bytes > pos ? (arena_bytes - pos) / step : 0;
        unsigned k = max_pkts - n < kMmsg ? max_pkts - n : kMmsg;
        if (room < k)
            k = static_cast<unsigned>(room);
        if (k == 0)
            break;
        uint8_t *bufs[kMmsg];
        for (unsigned i = 0; i < k; ++i)
            bufs[i] = h_arena + pos + static_cast<uint64_t>(i) * step;
        uint32_t len[kMmsg];
        bool trunc[kMmsg];
        const int r = recv_round(fd, bufs, mru, k, len, trunc);
        if (r == -ENOTSOCK) {
            sock = false;
            break;
        }
        if (r < 0)
            status = r;
        if (r <= 0)
            break;
        bool eof = false;
        for (int i = 0; i < r; ++i) {
            if (len[i] == 0) {
                eof = true;
                break;
            }
            if (trunc[i])
                continue;
            if (h_arena + pos != bufs[i])
                std::memmove(h_arena + pos, bufs[i], len[i]);
            take(len[i]);
        }
        if (eof || static_cast<unsigned>(r) < k) {
            *h_end = pos;
            return static_cast<int>(n);
        }
    }
    if (!sock) {
        NonBlocking nb(fd);
        if (!nb.ok())
            return RNS_E_IO;
        while (n < max_pkts && arena_bytes > pos && arena_bytes - pos >= mru) {
            const ssize_t r = read(fd, h_arena + pos, mru);
            if (r < 0) {
                if (errno == EINTR)
                    continue;
                if (errno != EAGAIN && errno != EWOULDBLOCK)
                    status = RNS_E_IO;
                break;
            }
            if (r == 0)
                break;
            if (static_cast<uint64_t>(r) > mru)
                continue;
            take(static_cast<uint32_t>(r));
        }
    }
    *h_end = pos;
    return (n == 0 && status) ? status : static_cast<int>(n);
}

int rns_io_recv_batch_chain(int fd, uint8_t *h_pool, uint32_t buf_bytes, uint32_t *h_free, uint32_t n_free,
                            uint32_t mru, uint32_t max_pkts, uint64_t *h_frag_off, uint32_t *h_frag_len,
                            uint32_t *h_first, uint32_t *n_frags_out, int timeout_ms)
{
    if (!h_frag_off || !h_frag_len || !h_first)
        return RNS_E_INVALID;
    struct {
        uint64_t *off;
        uint32_t *len, *first, buf_bytes;
        void begin() { first[0] = 0; }
        void frag(uint32_t j, uint32_t buf, uint32_t flen)
        {
            off[j] = static_cast<uint64_t>(buf) * buf_bytes;
            len[j] = flen;
        }
        void datagram(uint32_t i, uint32_t at, uint32_t cnt, uint32_t) { first[i + 1] = at + cnt; }
    } out = {h_frag_off, h_frag_len, h_first, buf_bytes};
    return recv_chain_loop(fd, h_pool, buf_bytes, h_free, n_free, mru, max_pkts, n_frags_out, timeout_ms, out);
}

int rns_io_recv_batch_pool(int fd, uint8_t *h_pool, uint32_t buf_log2, uint32_t *h_free, uint32_t n_free, uint32_t mru,
                           uint32_t max_pkts, uint16_t *h_len16, uint32_t *h_blk_first, uint32_t *n_frags_out,
                           int timeout_ms)
{
    if (!h_len16 || !h_blk_first || buf_log2 < 6 || buf_log2 > 15 || mru > 0xFFFFu)
        return RNS_E_INVALID;
    struct {
        uint16_t *len16;
        uint32_t *blk_first;
        void begin() {}
        void frag(uint32_t, uint32_t, uint32_t) {}  // h_free[j] is the descriptor
        void datagram(uint32_t i, uint32_t at, uint32_t, uint32_t len)
        {
            if ((i & 63u) == 0)
                blk_first[i >> 6] = at;
            len16[i] = static_cast<uint16_t>(len);
        }
    } out = {h_len16, h_blk_first};
    return recv_chain_loop(fd, h_pool, 1u << buf_log2, h_free, n_free, mru, max_pkts, n_frags_out, timeout_ms, out);
}

int rns_io_send_batch(int fd, const uint8_t *h_arena, const uint64_t *h_off, const uint32_t *h_len, uint32_t n)
{
    if (fd < 0 || (n && (!h_arena || !h_off || !h_len)))
        return RNS_E_INVALID;
    if (n > static_cast<uint32_t>(INT_MAX))
        n = static_cast<uint32_t>(INT_MAX);
    uint32_t i = 0;
    bool sock = true;
    while (sock && i < n) {  // sockets: sendmmsg, kMmsg datagrams per call
        const unsigned k = n - i < kMmsg ? n - i : kMmsg;
        struct mmsghdr mh[kMmsg];
        struct iovec iov[kMmsg];
        std::memset(mh, 0, sizeof(mh));
        for (unsigned j = 0; j < k; ++j) {
            iov[j].iov_base = const_cast<uint8_t *>(h_arena + h_off[i + j]);
            iov[j].iov_len = h_len[i + j];
            mh[j].msg_hdr.msg_iov = &iov[j];
            mh[j].msg_hdr.msg_iovlen = 1;
        }
        int w;
        do {
            w = sendmmsg(fd, mh, k, 0);
        } while (w < 0 && errno == EINTR);
        if (w < 0) {
            if (errno == ENOTSOCK && i == 0) {
                sock = false;
                break;
            }
            return i ? static_cast<int>(i) : RNS_E_IO;
        }
        i += static_cast<uint32_t>(w);
    }
    for (; i < n; ++i) {  // a TUN fd: one datagram per writev, like tun_send
        struct iovec v = {const_cast<uint8_t *>(h_arena + h_off[i]), h_len[i]};
        ssize_t w;
        do {
            w = writev(fd, &v, 1);
        } while (w < 0 && errno == EINTR);
        if (w < 0)
            return i ? static_cast<int>(i) : RNS_E_IO;
    }
    return static_cast<int>(n);
}

int rns_io_send_batch_chain(int fd, const uint8_t *h_arena, const uint64_t *h_frag_off, const uint32_t *h_frag_len,
                            const uint32_t *h_first, uint32_t n_pkts)
{
    if (fd < 0 || (n_pkts && (!h_arena || !h_first)))
        return RNS_E_INVALID;
    if (n_pkts > static_cast<uint32_t>(INT_MAX))
        n_pkts = static_cast<uint32_t>(INT_MAX);
    // every datagram's fragment range first (1..kChainIov fragments; an empty datagram would read
    // as end-of-stream on a SOCK_SEQPACKET peer): a malformed one sends nothing
    for (uint32_t i = 0; i < n_pkts; ++i) {
        const uint32_t f0 = h_first[i], f1 = h_first[i + 1];
        if (f1 <= f0 || f1 - f0 > kChainIov || !h_frag_off || !h_frag_len)
            return RNS_E_INVALID;
    }
    const auto frags = [&](uint32_t i, struct iovec *v) {
        const uint32_t f0 = h_first[i], nf = h_first[i + 1] - f0;
        for (uint32_t f = 0; f < nf; ++f) {
            v[f].iov_base = const_cast<uint8_t *>(h_arena + h_frag_off[f0 + f]);
            v[f].iov_len = h_frag_len[f0 + f];
        }
        return nf;
    };
    return send_chain_loop(fd, n_pkts, frags);
}

int rns_io_send_batch_pool(int fd, const uint8_t *h_pool, uint32_t buf_log2, const uint32_t *h_buf_idx,
                           const uint32_t *h_blk_first, const uint8_t *h_head_len8, const uint16_t *h_pay_len16,
                           uint32_t n_pkts)
{
    if (fd < 0 || buf_log2 < 8 || buf_log2 > 15 ||
        (n_pkts && (!h_pool || !h_buf_idx || !h_blk_first || !h_head_len8 || !h_pay_len16)))
        return RNS_E_INVALID;
    if (n_pkts > static_cast<uint32_t>(INT_MAX))
        n_pkts = static_cast<uint32_t>(INT_MAX);
    const uint32_t bbytes = 1u << buf_log2, bmask = bbytes - 1u;
    // every datagram first: a head (an empty one would read as end-of-stream on a SOCK_SEQPACKET peer)
    // and at most kChainIov fragments, else nothing is sent
    for (uint32_t i = 0; i < n_pkts; ++i)
        if (h_head_len8[i] == 0 || 1u + ((h_pay_len16[i] + bmask) >> buf_log2) > kChainIov)
            return RNS_E_INVALID;
    // first_i = h_blk_first[i / 64] + the buffers of the datagrams before i in its block; the loop asks
    // for the datagrams in ascending order with at most one step back (sendmmsg's short count), so the
    // running index restarts from the block's entry when i is not the next one
    uint32_t next = 0, at = 0;
    const auto frags = [&](uint32_t i, struct iovec *v) {
        if (i != next || (i & 63u) == 0) {
            at = h_blk_first[i >> 6];
            for (uint32_t k = i & ~63u; k < i; ++k)
                at += 1u + ((h_pay_len16[k] + bmask) >> buf_log2);
        }
        const uint32_t hl = h_head_len8[i], pay = h_pay_len16[i], npf = (pay + bmask) >> buf_log2;
        v[0].iov_base = const_cast<uint8_t *>(h_pool + (static_cast<uint64_t>(h_buf_idx[at]) << buf_log2) + (bbytes - hl));
        v[0].iov_len = hl;
        for (uint32_t f = 1; f <= npf; ++f) {
            v[f].iov_base = const_cast<uint8_t *>(h_pool + (static_cast<uint64_t>(h_buf_idx[at + f]) << buf_log2));
            v[f].iov_len = f < npf ? bbytes : pay - ((pay - 1u) & ~bmask);
        }
        at += 1u + npf;
        next = i + 1;
        return 1u + npf;
    };
    return send_chain_loop(fd, n_pkts, frags);
}

}  // extern "C"
