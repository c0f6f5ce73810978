// The rule instantiations of the mask predictor's score kernel (vb_mask_predict_rule: per-head energy
// bounds and the top-k mode in the epilogue), built as their own translation unit beside
// vb_predict.hip so that the two sets of kernels compile in parallel. See VB_PREDICT_RULE_TU there.
#define VB_PREDICT_RULE_TU 1
// the diagnostic device globals live in vb_predict.hip's unit only
#undef VB_PRED_TRACE
#define VB_PRED_TRACE 0
#undef VB_PRED_STAMPS
#define VB_PRED_STAMPS 0
#include "vb_predict.hip"
