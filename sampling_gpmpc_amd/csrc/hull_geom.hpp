// The two point predicates the hull kernels share (hull.hip builds the hulls with them, hull_query.hip tests points against
// the hulls with the same bits).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "min_index.hpp"   // finite1

namespace gpmpc {

__device__ __forceinline__ bool finite2(double x, double y) { return finite1(x) && finite1(y); }

// the cross product of the two difference vectors (a - c) x (b - c), ordinary FP64 with one fma
__device__ __forceinline__ double orient_d(double dax, double day, double dbx, double dby) { return fma(dax, dby, -(day * dbx)); }

__device__ __forceinline__ double orient(double cx, double cy, double ax, double ay, double bx, double by) {
    const double dax = ax - cx, day = ay - cy, dbx = bx - cx, dby = by - cy;
    return orient_d(dax, day, dbx, dby);
}

}  // namespace gpmpc
