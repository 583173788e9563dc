// GEMV instantiations: Q6_K (lm_head / ffn_down in Q4_K_M) and Q5_K (Q5_K_M files).
#include "gemv_impl.h"
namespace aios {
template GemvPlan gemv_pair<QT_Q6_K, QT_Q6_K>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_Q5_K, QT_Q5_K>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_Q5_K, QT_Q6_K>(const GemvArgs&, hipStream_t, int);
}  // namespace aios
