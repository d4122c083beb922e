// tile_rows.h — how the row-against-row kernels (silhouette.hip, row_knn.hip) fetch and widen the 16-byte piece of a
// row that one thread stages into an fp32 LDS image.  Not ABI.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "assign_common.h"

namespace rqsid {

template <int XF>
__device__ __forceinline__ uint4 load_raw(const void* base, int64_t row, int dim, int i4) {
  if constexpr (XF == RQSID_X_F32) {
    return reinterpret_cast<const uint4*>(static_cast<const float*>(base) + row * dim)[i4];
  } else {
    const uint2 w = reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(base) + row * dim)[i4];
    return make_uint4(w.x, w.y, 0u, 0u);
  }
}
template <int XF>
__device__ __forceinline__ float4 widen_raw(uint4 w) {
  float4 a;
  if constexpr (XF == RQSID_X_F32) {
    a = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
  } else if constexpr (XF == RQSID_X_F16) {
    // v_cvt_f32_f16: exact for every binary16 value, subnormals, infinities and NaNs included (these kernels run
    // in the default MODE, which keeps fp16 subnormals), so the image equals the widened fp32 row bit for bit
    const __half2 lo = *reinterpret_cast<const __half2*>(&w.x), hi = *reinterpret_cast<const __half2*>(&w.y);
    a = make_float4(__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi));
  } else {
    widen2<XF, true>(w.x, a.x, a.y);
    widen2<XF, true>(w.y, a.z, a.w);
  }
  return a;
}

}  // namespace rqsid
