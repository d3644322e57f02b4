// Token-major selective-scan kernels, BF16 I/O instantiation (see scan_tok.inc, scan_tok2.inc).
#include "scan_tok.inc"
#include "scan_tok2.inc"

namespace zigma {
int launch_scan_tok_bf16(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream) {
    return plan.family == ZIGMA_SCAN_KERNEL_TOK2 ? launch_tok2<BF16>(p, plan, stream) : launch_tok<BF16>(p, plan, stream);
}
}  // namespace zigma
