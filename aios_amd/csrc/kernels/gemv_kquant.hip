// GEMV instantiations: K-quant formats (Q4_K, Q5_K, Q6_K and the Q4_K_M mixed QKV pairs).
#include "gemv_impl.h"
namespace aios {
template GemvPlan gemv_pair<QT_Q4_K, QT_Q4_K>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_Q4_K, QT_Q6_K>(const GemvArgs&, hipStream_t, int);
}  // namespace aios
