// Reductions over the 64 lanes of a wavefront for any integer type: a butterfly of __shfl_xor, the result on every lane.  The type that
// is reduced is the argument's own; a caller whose operand is narrower than the sum it wants names the type (wave_sum<long long>(n)).
#pragma once
#include "bk_common.h"

template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
  for (int d = BK_WAVE / 2; d; d >>= 1) v += __shfl_xor(v, d, BK_WAVE);
  return v;
}
template <class T> __device__ __forceinline__ T wave_or(T v)
{
#pragma unroll
  for (int d = BK_WAVE / 2; d; d >>= 1) v |= __shfl_xor(v, d, BK_WAVE);
  return v;
}
template <class T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
  for (int d = BK_WAVE / 2; d; d >>= 1)
  {
    const T o = __shfl_xor(v, d, BK_WAVE);
    v = o < v ? o : v;
  }
  return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
  for (int d = BK_WAVE / 2; d; d >>= 1)
  {
    const T o = __shfl_xor(v, d, BK_WAVE);
    v = o > v ? o : v;
  }
  return v;
}
