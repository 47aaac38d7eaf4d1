// hm_math_common.h - the qualifier of the element formulas that both builds evaluate (hm_merge_math.h, hm_ops_math.h, hm_stats_math.h,
// hm_producer_math.h): one text for hipcc's device pass, its host pass and g++. The formulas use the <math.h> names, live in namespace hm
// and include no HIP header; where the builds perform different operations the header's top comment says so, under "DEVICE / HOST".
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HM_MATH_FN __host__ __device__ __forceinline__
#else
#define HM_MATH_FN inline
#endif
