// GEMV instantiations: 32-block formats (Q4_0, Q8_0) and 16-bit float weights (F16, BF16).
#include "gemv_impl.h"
namespace aios {
template GemvPlan gemv_pair<QT_Q4_0, QT_Q4_0>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_Q8_0, QT_Q8_0>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_F16, QT_F16>(const GemvArgs&, hipStream_t, int);
template GemvPlan gemv_pair<QT_BF16, QT_BF16>(const GemvArgs&, hipStream_t, int);
}  // namespace aios
