// popgen_plan.h -- what the popgen tools settle on the host before the GPU is asked (no HIP here): loci, windows, the kept windows.
#pragma once
#include "../../../include/poolgen_hip.h"
#include <stdexcept>
#include <string>
#include <vector>

// the reference's message where a tool finds no window (pi.rs:81, fst.rs:180)
constexpr const char *NO_WINDOWS =
    "There were no windows defined. Please check the sync file, the window size, slide size, and the minimum number of loci per window.";

struct PopgenPlan {
    std::vector<int64_t> locus_col; // count_loci (sync.rs:73-97) without the intercept entry: column starts, L + 1 of them ...
    std::vector<int32_t> chr_id;    // ... and each locus' coordinates
    std::vector<std::string> loc_chr;
    std::vector<uint64_t> loc_pos;
    std::vector<int64_t> wh, wt;           // define_sliding_windows: head and tail locus of every window
    bool reference_count = false;          // asked for: theta_watterson's own loop has run, on the same windows (checked), and kept ...
    std::vector<int64_t> wc, wseed, wslot; // ... these per window; empty otherwise
    // A window whose tail lies before its head (the stale tail of a ditched last slot; the reference's own gudmc test has one,
    // gudmc.rs:500-510) is an empty slice there.  keep: the others; kh .. kslot: wh .. wslot of those
    std::vector<int64_t> keep, kh, kt, kc, kseed, kslot;
    int64_t L() const { return (int64_t)loc_pos.size(); }
    int64_t nw() const { return (int64_t)wh.size(); }
};

// lab_chr / lab_pos: the labels of the matrix' columns behind the "intercept" entry at [0].  The two window loops are handed in: the
// CLI has them from the library, the GPU-free checker compiles them itself.
inline PopgenPlan plan_popgen(const std::vector<std::string> &lab_chr, const std::vector<uint64_t> &lab_pos, uint64_t window_size_bp,
                              uint64_t window_slide_size_bp, uint64_t min_loci_per_window, bool reference_count,
                              decltype(&pg_host_sliding_windows) sliding, decltype(&pg_host_watterson_windows) watterson) {
    PopgenPlan pl;
    pl.reference_count = reference_count;
    const int64_t p = (int64_t)lab_pos.size() - 1;
    for (int64_t c = 0; c < p; ++c)
        if (c == 0 || lab_chr[c] != lab_chr[c + 1] || lab_pos[c] != lab_pos[c + 1]) { // labels carry the intercept at [0]
            pl.locus_col.push_back(c);
            if (!pl.loc_chr.empty() && pl.loc_chr.back() == lab_chr[c + 1]) pl.chr_id.push_back(pl.chr_id.back());
            else pl.chr_id.push_back(pl.chr_id.empty() ? 0 : pl.chr_id.back() + 1);
            pl.loc_chr.push_back(lab_chr[c + 1]);
            pl.loc_pos.push_back(lab_pos[c + 1]);
        }
    pl.locus_col.push_back(p);
    const int64_t L = pl.L();
    pl.wh.resize(L); pl.wt.resize(L);
    const int64_t nw = sliding(pl.chr_id.data(), pl.loc_pos.data(), L, window_size_bp, window_slide_size_bp, min_loci_per_window,
                               pl.wh.data(), pl.wt.data());
    pl.wh.resize(nw); pl.wt.resize(nw);
    if (reference_count) { // the reference's own loop: the same windows, and what its count is made of
        std::vector<int64_t> h2(L), t2(L);
        pl.wc.resize(L); pl.wseed.resize(L); pl.wslot.resize(L);
        const int64_t nw2 = watterson(pl.chr_id.data(), pl.loc_pos.data(), L, window_size_bp, window_slide_size_bp, min_loci_per_window,
                                      h2.data(), t2.data(), pl.wc.data(), pl.wseed.data(), pl.wslot.data());
        h2.resize(nw2); t2.resize(nw2);
        if (h2 != pl.wh || t2 != pl.wt) throw std::runtime_error("internal error: the two window loops disagree"); // tajima_d.rs:46-47
        pl.wc.resize(nw); pl.wseed.resize(nw); pl.wslot.resize(nw);
    }
    for (int64_t w = 0; w < nw; ++w)
        if (pl.wh[w] <= pl.wt[w]) {
            pl.keep.push_back(w); pl.kh.push_back(pl.wh[w]); pl.kt.push_back(pl.wt[w]);
            if (reference_count) { pl.kc.push_back(pl.wc[w]); pl.kseed.push_back(pl.wseed[w]); pl.kslot.push_back(pl.wslot[w]); }
        }
    return pl;
}
