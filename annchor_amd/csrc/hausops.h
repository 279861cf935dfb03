// hausops.h -- what the two Hausdorff kernels share (hausdorff.hip: 1 .. 4 coordinates per point, hauswide.hip: 5 .. 512): the
// arguments and the exact min / max helpers.
#pragma once
#include "pairkern.h"

template <typename T> struct HausdorffArgs : PairArgs {
    const T *val;
    const int32_t *off, *len;   // counted in points
};

__device__ __forceinline__ double haus_xor_max(double v, int o)
{
    const int lo = __shfl_xor(__double2loint(v), o), hi = __shfl_xor(__double2hiint(v), o);
    return fmax(v, __hiloint2double(hi, lo));
}

// min of a running minimum and a fresh cost.  Neither is ever a NaN (finite input; a cost is a sum of squares, +inf at worst), so
// the instruction is given as it is: fmin() would first quieten the running minimum, one more float64 operation per cell.
__device__ __forceinline__ double haus_min(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ double haus_xor_min(double v, int o)
{
    const int lo = __shfl_xor(__double2loint(v), o), hi = __shfl_xor(__double2hiint(v), o);
    return haus_min(v, __hiloint2double(hi, lo));
}
