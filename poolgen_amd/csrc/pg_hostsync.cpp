// pg_hostsync.cpp -- pg_host_sync_parse: the host twin of the device sync parser (pg_sync.hip).  Plain C++ over the rules of
// pg_sync_line.h, a thread per share of the lines; no context, no GPU.  The checker of the device form and the baseline it is
// measured against.
#include "pg_common.h"
#include "pg_sync_line.h"
#include <algorithm>
#include <thread>

namespace {

struct SyncPart { // what one thread found in its share of the slab
    std::vector<uint32_t> counts;
    std::vector<uint64_t> pos;
    std::vector<int64_t> off;
    std::vector<int32_t> clen;
    int64_t data_lines = 0;
    uint64_t err = PG_SYNC_NO_ERR;
};

// 0 skipped, 1 kept, or minus a pg_sync_reason; n_ref: the pools every line must have
int sync_host_line(const unsigned char *line, int64_t len, int64_t off, int n_ref, SyncPart &P) {
    if (len == 0) return -PG_SYNC_E_EMPTY;
    if (line[0] == '#') return 0;
    ++P.data_lines;
    if (len > 0x7fffffffLL) return -PG_SYNC_E_LONG;
    int64_t tabs = 0, t1 = -1, t2 = -1, t3 = -1;
    for (int64_t i = 0; i < len; ++i)
        if (line[i] == '\t') {
            ++tabs;
            if (tabs == 1) t1 = i;
            else if (tabs == 2) t2 = i;
            else if (tabs == 3) t3 = i;
        }
    uint64_t pos = 0;
    const bool pos_ok = tabs >= 2 && pg_sync_pos(line + t1 + 1, t2 - t1 - 1, &pos);
    const int head = pg_sync_head(tabs, pos_ok);
    if (head != 1) return head;
    const int64_t m = tabs - 2;
    const int64_t mm = std::min<int64_t>(m, n_ref);
    int err = m != n_ref ? PG_SYNC_E_POOLS : 0;
    const size_t at = P.counts.size();
    int64_t b = t3 + 1;
    for (int64_t j = 0; j < mm; ++j) {
        const void *t = std::memchr(line + b, '\t', (size_t)(len - b));
        const int64_t e = t ? (int64_t)(static_cast<const unsigned char *>(t) - line) : len;
        PgSyncPool pl;
        pg_sync_pool(line + b, e - b, &pl);
        err = pg_sync_min_code(err, pl.err);
        const uint32_t six[6] = {pl.c0, pl.c1, pl.c2, pl.c3, pl.c4, pl.c5};
        P.counts.insert(P.counts.end(), six, six + 6);
        b = e + 1;
    }
    if (err) {
        P.counts.resize(at);
        return -err;
    }
    P.pos.push_back(pos);
    P.off.push_back(off);
    P.clen.push_back((int32_t)t1);
    return 1;
}

struct SyncLines { // the lines of a slab, one after the other
    const unsigned char *text;
    int64_t bytes;
    // the line that starts at s: its length without newline and '\r'; returns the start of the next one
    int64_t at(int64_t s, int64_t *len) const {
        const void *nl = std::memchr(text + s, '\n', (size_t)(bytes - s));
        const int64_t e = nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) : bytes;
        *len = e - s;
        if (*len > 0 && text[e - 1] == '\r') --*len;
        return e + 1;
    }
    int64_t start_at_or_after(int64_t x) const { // the first line start >= x
        if (x <= 0) return 0;
        if (x >= bytes) return bytes;
        const void *nl = std::memchr(text + x - 1, '\n', (size_t)(bytes - (x - 1)));
        return nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) + 1 : bytes;
    }
};

void sync_host_share(const SyncLines &T, int64_t lo, int64_t hi, int n_ref, SyncPart &P) {
    int64_t s = T.start_at_or_after(lo);
    const int64_t end = T.start_at_or_after(hi);
    while (s < end) {
        int64_t len;
        const int64_t next = T.at(s, &len);
        const int st = sync_host_line(T.text + s, len, s, n_ref, P);
        if (st < 0) {
            P.err = std::min(P.err, pg_sync_err_key(s, -st));
            return; // (later lines of this share cannot come first)
        }
        s = next;
    }
}

} // namespace

extern "C" int pg_host_sync_parse(const char *text_, int64_t bytes, int expect_n, uint32_t *counts, uint64_t *pos, int64_t *line_off,
                                  int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_sync_info *info, int n_threads) {
    if (!info) return PG_ERR_INVALID;
    *info = pg_sync_info{0, 0, -1, 0, 0};
    if (bytes < 0 || (bytes > 0 && !text_) || expect_n < 0 || expect_n > PG_SYNC_MAX_POOLS || cap_loci < 0 || cap_counts < 0) return PG_ERR_INVALID;
    if (bytes == 0) return PG_OK;
    const SyncLines T{reinterpret_cast<const unsigned char *>(text_), bytes};
    // the first line that does not start with '#' fixes the pool count
    uint64_t err = PG_SYNC_NO_ERR;
    int n_first = 0;
    for (int64_t s = 0; s < bytes;) {
        int64_t len;
        const int64_t next = T.at(s, &len);
        if (T.text[s] != '#') {
            int64_t tabs = 0;
            for (int64_t i = 0; i < len; ++i) tabs += T.text[s + i] == '\t' ? 1 : 0;
            const int code = pg_sync_first_line((int)std::min<int64_t>(tabs, PG_SYNC_TAB_CAP), expect_n, &n_first);
            if (code) err = pg_sync_err_key(s, code);
            break;
        }
        s = next;
    }
    const int n_ref = expect_n > 0 ? expect_n : std::max(1, std::min(n_first, PG_SYNC_MAX_POOLS));
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, bytes / 4096 + 1));
    const int64_t each = (bytes + parts - 1) / parts;
    std::vector<SyncPart> P(parts);
    {
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t)
            th.emplace_back([&, t] { sync_host_share(T, std::min(bytes, t * each), std::min(bytes, (t + 1) * each), n_ref, P[t]); });
        sync_host_share(T, 0, std::min(bytes, each), n_ref, P[0]);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < parts; ++t) {
        err = std::min(err, P[t].err);
        info->data_lines += P[t].data_lines;
    }
    if (err != PG_SYNC_NO_ERR) {
        info->err_line_off = (int64_t)(err >> 8);
        info->err_reason = (int32_t)(err & 0xff);
        return PG_ERR_INVALID;
    }
    int64_t kept = 0;
    for (int t = 0; t < parts; ++t) kept += (int64_t)P[t].pos.size();
    info->kept = kept;
    info->n_pools = n_first;
    const int64_t need_counts = kept * info->n_pools * 6;
    if (kept > cap_loci || need_counts > cap_counts) return PG_ERR_INVALID;
    if (kept == 0) return PG_OK;
    if (!pos || !line_off || !chrom_len || !counts) return PG_ERR_INVALID;
    int64_t at = 0;
    for (int t = 0; t < parts; ++t) {
        const int64_t k = (int64_t)P[t].pos.size();
        if (!k) continue;
        std::memcpy(pos + at, P[t].pos.data(), sizeof(uint64_t) * k);
        std::memcpy(line_off + at, P[t].off.data(), sizeof(int64_t) * k);
        std::memcpy(chrom_len + at, P[t].clen.data(), sizeof(int32_t) * k);
        std::memcpy(counts + at * info->n_pools * 6, P[t].counts.data(), sizeof(uint32_t) * P[t].counts.size());
        at += k;
    }
    return PG_OK;
}
