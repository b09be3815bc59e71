#pragma once
// A dnagpu_chain_plan put together step by step (dna_adjust::PrepareLockstepChains, dna_adjust::EnsureRigorousPlan): the steps' lists
// live here, and the dnagpu_chain_step array that points into them is made when the plan is.
#include <cstdint>
#include <vector>
#include "../../../include/dnagpu.h"

struct chain_step_data {
    uint32_t n_stn = 0;                                  // stations of the step's system
    int n_src = 0;
    const dnagpu_matrix* src[3] = {};
    int junction[3] = {};
    std::vector<uint32_t> pos[3];                        // where source q's stations go in the step's system
    std::vector<uint32_t> est_blk, est_idx;              // the linearisation point (empty: none)
    std::vector<uint32_t> keep, con_stn;
    std::vector<double> con_w9;
    dnagpu_matrix* out = nullptr;
    int out_junction = 0;
    int matrix_only = 0;

    void add_source(const dnagpu_matrix* m, int junc, const std::vector<uint32_t>& p) {
        src[n_src] = m;
        junction[n_src] = junc;
        pos[n_src++] = p;
    }
    dnagpu_chain_step view() const {
        dnagpu_chain_step st{};
        st.n_stn = n_stn;
        st.est_blk = ptr(est_blk);
        st.est_idx = ptr(est_idx);
        st.n_src = n_src;
        for (int q = 0; q < n_src; ++q) st.src[q] = {src[q], junction[q], ptr(pos[q]), pos[q].size()};
        st.con_stn = ptr(con_stn);
        st.con_w9 = ptr(con_w9);
        st.n_con = con_stn.size();
        st.keep = ptr(keep);
        st.n_keep = keep.size();
        st.out = out;
        st.out_junction = out_junction;
        st.matrix_only = matrix_only;
        return st;
    }
    template <class T>
    static const T* ptr(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
};

class chain_plan_builder {
public:
    // returns what eliminating all but the step's kept stations costs
    double add_step(chain_step_data&& d) {
        const double n = 3.0 * (double)d.n_stn, nj = 3.0 * (double)d.keep.size(), ni = n - nj;
        steps_.push_back(std::move(d));
        return ni * ni * ni / 3.0 + ni * ni * nj + ni * nj * nj;
    }
    void close_batch() { batch_first_.push_back((uint32_t)steps_.size()); }
    chain_step_data& step(size_t i) { return steps_[i]; }
    size_t steps() const { return steps_.size(); }
    size_t batches() const { return batch_first_.size() - 1; }
    int create(dnagpu_ctx* ctx, double budget, dnagpu_chain_plan** plan) const {
        std::vector<dnagpu_chain_step> st;
        for (const chain_step_data& d : steps_) st.push_back(d.view());
        return dnagpu_chain_plan_create(ctx, st.size(), st.data(), batches(), batch_first_.data(), budget, plan);
    }

private:
    std::vector<chain_step_data> steps_;
    std::vector<uint32_t> batch_first_{0};
};
