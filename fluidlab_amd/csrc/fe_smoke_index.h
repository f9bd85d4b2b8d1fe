// fe_smoke_index.h -- one axis of the trilinear back-trace index of fe_smoke.h (sm_trilerp), defined for every float.
//
// The back-traced point p of a cell is p0 - dt * v: with a non-finite or huge v in the frame, (int)floorf(p - 0.5f) is undefined and
// base + 1 can overflow before it is clamped.  p is therefore clamped into [-2^30, 2^30] before anything is converted: the comparisons
// are written so that NaN goes to the lower bound (no reliance on fminf / fmaxf), both bounds and bound - 0.5f are exact in fp32, and
// base + 1 <= 2^30 fits an int.  For every finite |p| <= 2^30 the clamp is the identity, so base and f are the bits they always were;
// at and beyond the bounds f is 0 (p - 0.5f rounds to an integer there) and both cells are the grid's edge cell.
// Plain __host__ __device__ code: tests/csrc/smoke_index_test.hip compiles it for the host and for the GPU.
#ifndef FE_SMOKE_INDEX_H
#define FE_SMOKE_INDEX_H

#define FE_SM_P_MAX 1073741824.0f            /* 2^30 */

// p: a position in cell units along one axis of an n-cell grid.  base = floor(p - 0.5), f = the fraction towards base + 1,
// c0 / c1 = base / base + 1 clamped into [0, n - 1].
__host__ __device__ inline void sm_tri_axis(float p, int n, int& base, float& f, int& c0, int& c1) {
    const float lo = -FE_SM_P_MAX, hi = FE_SM_P_MAX;
    p = p > lo ? (p < hi ? p : hi) : lo;
    base = (int)floorf(p - 0.5f);
    f = p - 0.5f - (float)base;
    const int b1 = base + 1;
    c0 = base < 0 ? 0 : (base > n - 1 ? n - 1 : base);
    c1 = b1 < 0 ? 0 : (b1 > n - 1 ? n - 1 : b1);
}

#endif /* FE_SMOKE_INDEX_H */
