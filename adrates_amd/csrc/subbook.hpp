// Sub-books of a scenario revaluation (subbook.hip): the chunk plan, the fixed-order sum per sub-book and the tail
// measures and their allocation; shared by scenario_pv.hip, credit_scenario_pv.hip and yoy_scenario_pv.hip.  The whole book's sum, which subbook.hip holds too, is
// declared in scenario_common.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace adr {
namespace sub {

// The plan of B sub-books with C chunks in all, B + 1 + 2 C int64 (adr_scenario_subbook_plan fills it):
//   plan[0 .. B]            chunk_off: sub-book b owns the chunks chunk_off[b] .. chunk_off[b + 1] (chunk_off[B] = C)
//   plan[B + 1 + 2 c, + 1]  the first trade of chunk c and the one after its last
struct Plan {
    const int64_t* chunk_off;
    const int64_t* bounds;
};
inline Plan plan_view(const int64_t* plan, int64_t B) { return Plan{plan, plan + B + 1}; }

inline int64_t max_chunks(int64_t n, int64_t B, int chunk) { return (n + chunk - 1) / chunk + B; }

// ADR_ERR_INVALID naming the sub-book unless sub_off runs from 0 to n without decreasing.
int check_offsets(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off);

// check_offsets, then `plan` resized and filled (adr_scenario_subbook_plan).
int build_plan(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off, std::vector<int64_t>& plan);

// sub_pv[b][e] = the fixed-order sum of sub-book b's chunk rows: its chunk j to slot j % 64 in order, then a halving
// tree.  Chunk counts beyond chunk_cap are cut there (work holds that many rows).
hipError_t enqueue_sum(const double* work, const int64_t* chunk_off, int64_t chunk_cap, int64_t B, int S, double* sub_pv,
                       hipStream_t stream);
void reduce_subbooks(const double* work, const int64_t* chunk_off, int64_t B, int64_t S, double* sub_pv);

// var[b], es[b] of rows[b][S_tot] (adr_scenario_tail's rule); k and the width have been checked.
hipError_t enqueue_tail(const double* rows, int64_t B, int S_tot, int base_col, int k, double* var, double* es, hipStream_t stream);
int check_tail(const std::string& w, int64_t B, int S_tot, int base_col, int k);

// The tail allocation of rows[b][S_tot] (adr_scenario_tail_alloc's rule): the firm's var and es and every row's
// components; `work` holds S_tot doubles; k and the width have been checked.  Three kernels on `stream`.
hipError_t enqueue_alloc(const double* rows, int64_t B, int S_tot, int base_col, int k, double* var_tot, double* es_tot,
                         double* comp_var, double* comp_es, double* work, hipStream_t stream);
int check_alloc(const std::string& w, int64_t B, int S_tot, int base_col, int k);

}  // namespace sub
}  // namespace adr
