// The mask predictor's rule instantiations (vb_mask_predict_rule: per-head bounds, top-k mode): the
// 12 kRule score kernels, every head dim, dtype and sampling density, in the long form only. A
// translation unit of their own so that the two halves of the predictor's kernels compile side by
// side (vb_predict.hip holds the other 16). Defines launch_predict_rule and nothing else with
// external linkage; the diagnostic hooks stay empty here (see vb_predict_kernel.hpp).
#include "vb_predict_kernel.hpp"

namespace vb {

template <int D, class T>
static int launch_predict_rule_dt(const PredParams& p, int keep, hipStream_t s, hipEvent_t ev) {
  if (keep == 16) return launch_predict<D, T, true, 16, true>(p, s, ev);
  if (keep == 64) return launch_predict<D, T, true, 64, true>(p, s, ev);
  return launch_predict<D, T, true, 32, true>(p, s, ev);
}

int launch_predict_rule(const PredParams& p, int dtype, int keep, hipStream_t s, hipEvent_t ev) {
  const bool bf = dtype == VB_DTYPE_BF16;
  if (p.D == 64) return bf ? launch_predict_rule_dt<64, BF16>(p, keep, s, ev) : launch_predict_rule_dt<64, F16>(p, keep, s, ev);
  return bf ? launch_predict_rule_dt<128, BF16>(p, keep, s, ev) : launch_predict_rule_dt<128, F16>(p, keep, s, ev);
}

}  // namespace vb
