// The score of every int8 kernel (store scan, dual scan, threshold sample),
// one rounding per step whatever the surrounding code lets the compiler
// contract: p = float(sum) * row scale (the int32 -> float conversion is
// exact, |sum| < 2^24 for D <= 1024), score = fma(al, p, bias) with
// al = alpha * query scale. Every int8 epilogue takes its scores from these
// two, so any two kernels give a row bit-identical scores.
#pragma once
#include "lzk_common.h"

__device__ __forceinline__ float i8_prod(int v, float rs) { return __fmul_rn((float)v, rs); }
__device__ __forceinline__ float i8_score(float al, float p, float b) { return __fmaf_rn(al, p, b); }
