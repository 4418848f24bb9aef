// The model value the resident-PL likelihood compares with an observation, before the magnitude offset is added: one
// definition, shared by the kernels that score PL rows in HBM (likelihood.hip) and by the posterior-predictive band
// (predictive.hip), so that "the values the likelihood compared" are the same bits in both.
#pragma once
#include <float.h>
#include <math.h>

#include <hip/hip_runtime.h>

namespace trpl {

// re-dimensionalised PL -> optional self-normalisation to the row's t = 0 value -> clamp at DBL_MIN -> log10
// (bayeslib.py:150-157)
template <typename T>
__device__ __forceinline__ double log_pl(T v, T v0, bool normalize, bool f32_staging)
{
    if (f32_staging) {                       // the reference's float32 plI buffer (bayeslib.py:137)
        float f = (float)v;
        if (normalize) f = f / (float)v0;
        if ((double)f < DBL_MIN) f = (float)DBL_MIN;
        return (double)(float)log10((double)f);
    }
    double d = (double)v;
    if (normalize) d = d / (double)v0;
    if (d < DBL_MIN) d = DBL_MIN;
    return log10(d);
}

}  // namespace trpl
