// result_writer.h -- --result-writer gpu: the result rows of the GWAS analyses formatted by the GPU that computed them
// (pg_result_rows_dev, pg_kinship_rows_dev); --popgen-writer gpu takes the same format-and-write loop (text()).  The statistics stay where the operator left them; only their text comes back, into
// pinned memory, and is appended to the file the caller has opened (and removes when anything on the way throws).
#pragma once
#include "../../../include/poolgen_hip.h"
#include "gpu_mem.h"
#include "host_util.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace pgh {

constexpr int64_t RESULT_SLAB_BYTES = (int64_t)256 << 20; // the byte budget behind the default of --result-slab-rows
constexpr int64_t RESULT_ROW_TYPICAL = 128;               // bytes of a row for that default: label, Pheno_j and two cells of ordinary length

inline int64_t result_slab_rows(int flag) { return flag > 0 ? flag : RESULT_SLAB_BYTES / RESULT_ROW_TYPICAL; }

class DeviceResultWriter {
public:
    // who: the flag's word, "result" (--result-writer) or "popgen" (--popgen-writer): in the messages and in the timing line
    explicit DeviceResultWriter(const char *who = "result") : who_(who) {}
    DeviceResultWriter(const DeviceResultWriter &) = delete;
    DeviceResultWriter &operator=(const DeviceResultWriter &) = delete;
    ~DeviceResultWriter() {
        if (std::getenv("PGH_TIMING") && text_bytes_ > 0)
            std::fprintf(stderr, "poolgen: %s writer on the GPU, %.1f MB of text: labels up %.3f s, format calls %.3f s, D2H of the text %.3f s, file writes %.3f s\n",
                         who_, text_bytes_ / 1e6, t_labels_, t_format_, t_d2h_, t_write_);
    }
    // The labels of a piece, up once: chromosome id and position per locus, the name table (SyncBatch's).
    void set_locus_labels(const std::vector<int32_t> &chrom_id, const std::vector<uint64_t> &pos, const std::vector<std::string> &names, int64_t L) {
        const double t0 = now();
        chrom_dev_.reserve(sizeof(int32_t) * (size_t)L, "the labels of a piece");
        pos_dev_.reserve(sizeof(uint64_t) * (size_t)L, "the labels of a piece");
        hip_ok(hipMemcpy(chrom_dev_.get(), chrom_id.data(), sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice), "H2D labels");
        hip_ok(hipMemcpy(pos_dev_.get(), pos.data(), sizeof(uint64_t) * (size_t)L, hipMemcpyHostToDevice), "H2D labels");
        set_names(names);
        t_labels_ += now() - t0;
    }
    // The labels of the matrix' columns (kinship rows): chromosome id, position, allele id per column.
    void set_column_labels(const std::vector<int32_t> &chrom_id, const std::vector<uint64_t> &pos, const std::vector<int32_t> &allele,
                           const std::vector<std::string> &names) {
        const double t0 = now();
        const size_t p = chrom_id.size();
        chrom_dev_.reserve(sizeof(int32_t) * (p + 1), "the labels of the columns");
        pos_dev_.reserve(sizeof(uint64_t) * (p + 1), "the labels of the columns");
        allele_dev_.reserve(sizeof(int32_t) * (p + 1), "the labels of the columns");
        hip_ok(hipMemcpy(chrom_dev_.get(), chrom_id.data(), sizeof(int32_t) * p, hipMemcpyHostToDevice), "H2D labels");
        hip_ok(hipMemcpy(pos_dev_.get(), pos.data(), sizeof(uint64_t) * p, hipMemcpyHostToDevice), "H2D labels");
        hip_ok(hipMemcpy(allele_dev_.get(), allele.data(), sizeof(int32_t) * p, hipMemcpyHostToDevice), "H2D labels");
        set_names(names);
        t_labels_ += now() - t0;
    }
    // The rows of the L loci whose labels are set, from the operator's slot-major outputs on the device, appended to fo.
    void locus_rows(pg_ctx *ctx, int op, int64_t L, int k, const int32_t *n_out_dev, const int32_t *ids_dev, const double *mf_dev,
                    const double *stat_dev, const double *pv_dev, FILE *fo) {
        format_and_write(ctx, fo, [&](char *text, int64_t cap, int64_t *need) {
            return pg_result_rows_dev(ctx, op, L, k, n_out_dev, ids_dev, mf_dev, stat_dev, pv_dev, chrom_dev_.get(), pos_dev_.get(), names_dev_.get(),
                                      off_dev_.get(), n_chrom_, text, cap, need);
        });
    }
    // Rows [row0, row0 + rows) of the k * p kinship rows, appended to fo.
    void kinship_rows(pg_ctx *ctx, int64_t p, int k, int64_t row0, int64_t rows, const double *beta_dev, const double *pval_dev, FILE *fo) {
        format_and_write(ctx, fo, [&](char *text, int64_t cap, int64_t *need) {
            return pg_kinship_rows_dev(ctx, p, k, row0, rows, beta_dev, pval_dev, chrom_dev_.get(), pos_dev_.get(), allele_dev_.get(), names_dev_.get(),
                                       off_dev_.get(), n_chrom_, text, cap, need);
        });
    }
    // Any other formatter of the library's conventions: call(text_dev, cap, &need) formats into the writer's buffer (or asks for
    // a larger one); its text is appended to fo.
    template <class Call>
    void text(pg_ctx *ctx, FILE *fo, Call call) { format_and_write(ctx, fo, call); }

private:
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void set_names(const std::vector<std::string> &names) {
        std::string text;
        std::vector<int32_t> off{0};
        for (const std::string &s : names) { text += s; off.push_back((int32_t)text.size()); }
        names_dev_.reserve(text.size() + 1, "the chromosome names");
        off_dev_.reserve(sizeof(int32_t) * off.size(), "the chromosome names");
        if (!text.empty()) hip_ok(hipMemcpy(names_dev_.get(), text.data(), text.size(), hipMemcpyHostToDevice), "H2D labels");
        hip_ok(hipMemcpy(off_dev_.get(), off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice), "H2D labels");
        n_chrom_ = (int)names.size();
    }
    template <class Call>
    void format_and_write(pg_ctx *ctx, FILE *fo, Call call) {
        double t0 = now();
        int64_t need = 0;
        for (int attempt = 0;; ++attempt) { // the buffer of the turn before serves this one; when it does not, the size is known
            const int rc = call(text_dev_.get(), cap_, &need);
            if (rc == PG_OK) break;
            if (attempt > 0 || need <= cap_) throw std::runtime_error("--" + std::string(who_) + "-writer gpu: " + pg_last_error(ctx));
            cap_ = need + need / 8;
            text_dev_.reset((size_t)cap_, "the text of the result rows");
        }
        if (pg_synchronize(ctx) != PG_OK) throw std::runtime_error("--" + std::string(who_) + "-writer gpu: " + pg_last_error(ctx));
        t_format_ += now() - t0; t0 = now();
        if (need == 0) return;
        char *pin = static_cast<char *>(pin_.reserve((size_t)need));
        if (!pin) throw std::runtime_error("out of pinned memory for the text of the result rows");
        hip_ok(hipMemcpy(pin, text_dev_.get(), (size_t)need, hipMemcpyDeviceToHost), "D2H of the text of the result rows");
        t_d2h_ += now() - t0; t0 = now();
        if (std::fwrite(pin, 1, (size_t)need, fo) != (size_t)need) throw std::runtime_error("write failed (disk full?)");
        t_write_ += now() - t0;
        text_bytes_ += (double)need;
    }
    DeviceBuf<int32_t> chrom_dev_, allele_dev_, off_dev_;
    DeviceBuf<uint64_t> pos_dev_;
    DeviceBuf<char> names_dev_, text_dev_;
    PinnedBuf pin_;
    int64_t cap_ = 0;
    int n_chrom_ = 0;
    const char *who_;
    double t_labels_ = 0, t_format_ = 0, t_d2h_ = 0, t_write_ = 0, text_bytes_ = 0;
};

} // namespace pgh
