// pg_hostwindows.cpp -- the reference's two window loops on the host (pg_host_sliding_windows, pg_host_watterson_windows of
// include/poolgen_hip.h): plain C++ with no HIP in it, so that the CLI's GPU-free checker (host/hostcheck.cpp) compiles this
// file as it is.
#include "../../include/poolgen_hip.h"
#include <cstddef>
#include <vector>

// define_sliding_windows (base/helpers.rs:294-403)
extern "C" int64_t pg_host_sliding_windows(const int32_t *chr, const uint64_t *pos, int64_t l, uint64_t window_size_bp,
                                           uint64_t window_slide_size_bp, uint64_t min_loci_per_window, int64_t *out_head,
                                           int64_t *out_tail) {
    if (l <= 0 || !chr || !pos || !out_head || !out_tail) return 0;
    std::vector<int64_t> head{0}, tail{0};
    std::vector<uint64_t> cnt{1};
    bool next_found = false;
    int64_t next_head = 0;
    for (int64_t i = 1; i < l; ++i) {
        const int64_t h = head.back();
        if (chr[i] != chr[h] || pos[i] > pos[h] + window_size_bp) {
            if (next_found) i = next_head;                 // the next window starts inside the ending one (:331-335)
            if (cnt.back() >= min_loci_per_window) { head.push_back(i); tail.push_back(i); cnt.push_back(1); }
            else { head.back() = i; cnt.back() = 1; }     // too few loci: the slot is reused, its tail stays (:350-357)
            next_found = false;
        } else {
            tail.back() = i;
            cnt.back() += 1;
            if (!next_found && pos[i] >= pos[h] + window_slide_size_bp) { next_found = true; next_head = i; }
        }
    }
    int64_t no = 0;
    for (size_t w = 0; w < head.size(); ++w)               // windows ending where the previous one ends are dropped (:380-391)
        if (w == 0 || tail[w] != out_tail[no - 1]) { out_head[no] = head[w]; out_tail[no] = tail[w]; ++no; }
    return no;
}

// theta_watterson's own copy of that loop (watterson_theta.rs:56-164), with what it keeps per window besides head and tail
extern "C" int64_t pg_host_watterson_windows(const int32_t *chr, const uint64_t *pos, int64_t l, uint64_t window_size_bp,
                                             uint64_t window_slide_size_bp, uint64_t min_loci_per_window, int64_t *out_head,
                                             int64_t *out_tail, int64_t *out_cov, int64_t *out_seed, int64_t *out_slot) {
    if (l <= 0 || !chr || !pos || !out_head || !out_tail || !out_cov || !out_seed || !out_slot) return 0;
    std::vector<int64_t> head{0}, tail{0}, seed{0};
    std::vector<uint64_t> cnt{1};
    bool next_found = false;
    int64_t next_head = 0;
    for (int64_t i = 1; i < l; ++i) {
        const int64_t h = head.back();
        if (chr[i] != chr[h] || pos[i] > pos[h] + window_size_bp) {
            if (next_found) i = next_head;                                                     // :89-93
            if (cnt.back() >= min_loci_per_window) { head.push_back(i); tail.push_back(i); cnt.push_back(1); seed.push_back(i); } // :100-109
            else { head.back() = i; cnt.back() = 1; seed.back() = (int64_t)head.size() - 1; } // polymorphic_loci_per_pool(.., i_), :113-119
            next_found = false;
        } else {
            tail.back() = i;
            cnt.back() += 1; // and polymorphic[i_] += polymorphic_loci_per_pool(.., i_): the slot's index again (:127-137)
            if (!next_found && pos[i] >= pos[h] + window_slide_size_bp) { next_found = true; next_head = i; }
        }
    }
    int64_t no = 0;
    for (size_t w = 0; w < head.size(); ++w) // :152-164
        if (w == 0 || tail[w] != out_tail[no - 1]) {
            out_head[no] = head[w]; out_tail[no] = tail[w]; out_cov[no] = (int64_t)cnt[w]; out_seed[no] = seed[w]; out_slot[no] = (int64_t)w;
            ++no;
        }
    return no;
}
