// Stable segmented sort of 64-bit keys (k17_coco_eval.hip): per segment, 1024-element tiles sorted in LDS (bitonic) by
// (key, position), then merge passes of sorted runs.  K17 sorts its kept detections with it (keys made from the scores in the
// tile pass); K18 hands it keys it has written itself.  Internal to the library, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pod {

// ascending total order of doubles as unsigned 64-bit keys (-0.0 == 0.0, as numpy / torch compare)
__device__ inline uint64_t asc_key(double s) {
    if (s == 0.0) s = 0.0;
    const uint64_t u = (uint64_t)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline double asc_key_value(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// Sorts segment s = [seg_off[s], seg_off[s + 1]) of n_seg segments (the longest max_seg) stably by key.  desc_scores != NULL:
// the keys are made from those fp64 scores, descending (K17); NULL: key0 holds them.  idx = global position.  key0 / idx0 and
// key1 / idx1 are ping-pong buffers of the total length; *keys / *order point at the one holding the result.  Returns 0 or POD_E_LAUNCH.
int segsort(const int64_t* seg_off, int32_t n_seg, int32_t max_seg, const double* desc_scores, uint64_t* key0, int32_t* idx0,
            uint64_t* key1, int32_t* idx1, uint64_t** keys, int32_t** order, hipStream_t st);

}  // namespace pod
