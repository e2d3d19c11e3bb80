// The ordered tail select of tail_select.hip as tail_order.hip composes it (adr_scenario_tail_alloc_select*): the checks,
// the scratch and the chain on a stream, and the CPU twin.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace adr {
namespace tsel {

// ADR_OK, or the refusal of adr_scenario_tail_order* in w's name: adr_scenario_tail_select's, with the limit on k at
// ADR_SCENARIO_ALLOC_MAX.
int check_order(const std::string& w, int64_t B, int S_tot, int base_col, int k);

// The scratch of enqueue_order in bytes, a multiple of 16.
size_t order_work_bytes(int64_t B, int S_tot, int k);

// order[B][k], var[B], es[B] of rows[B][S_tot] on `stream`; every pointer is device memory, `work` holds
// order_work_bytes(B, S_tot, k) and is 16-byte aligned.  Sizes have been checked.
int enqueue_order(const std::string& w, const double* rows, int64_t B, int S_tot, int base_col, int k, int64_t* order, double* var,
                  double* es, void* work, hipStream_t stream);

// The CPU twin: std::nth_element on the (key, index) pairs, a sort of the first k, the same sums.
void order_host(const double* rows, int64_t B, int S_tot, int base_col, int k, int64_t* order, double* var, double* es);

}  // namespace tsel
}  // namespace adr
