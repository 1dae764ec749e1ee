// L-BFGS stage after Adam for gfx950 (hpv_lbfgs_step): the optimiser's vectors -- theta, theta0, g, d and the rings S, Y, rho -- live
// on the device; the host sees scalars only (LbfgsArgs::scal) and runs the strong-Wolfe search over them (hpv_linesearch.h).
//   k_lbfgs_direction   two-loop recursion over the live pairs of the ring, H_diag of the newest one; also g . d, max|g|, sum|g|, max|d|
//   k_lbfgs_trial       theta = theta0 + t d into the handle's live parameter buffer
//   k_lbfgs_probe       after a backward pass: {loss, g_new . d, max|g_new|} from the packed buffer; the gradient is kept aside
//   k_lbfgs_push        s = t d, y = g_new - g: stored at the ring's head when y . s > HPV_LBFGS_YS_MIN, skipped and counted otherwise;
//                       then g = g_new, theta0 = theta
// The three kernels that reduce run as ONE workgroup of LB_THREADS threads: the vectors have a few thousand entries (P = 921 .. 4417 for
// the networks of the drivers), the recursion is a chain of 2 n_hist dependent dot products, and between two of them stands one
// workgroup barrier instead of a launch.  Thread j owns the entries j, j + LB_THREADS, ..: it is the only one that reads or writes
// them, so the running vector q needs no barrier of its own, and every update pass already gathers the partial sums of the NEXT dot
// product.
//
// Reproducibility (bitwise, call to call): the summation order of every dot product is a function of P alone --
//   thread:     its entries in ascending order;
//   wave:       the fixed butterfly of hpv_lane.h (group_reduce<64>: VALU only, the same tree in every lane, all 64 lanes active);
//   workgroup:  the waves' results in wave order, by every thread alike.
// No atomics, no floating-point order that depends on timing; P is a run-time value with no divisibility assumption.
#include "hpv_internal.h"
#include "hpv_lane.h"

#define LB_THREADS 1024
#define LB_WAVES (LB_THREADS / 64)

namespace {

struct LbMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };
struct LbSum { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };

// Reduction over the workgroup, the result in every thread.  red: [2][LB_WAVES]; consecutive calls alternate `flip`, so that ONE
// barrier per call is enough: whoever writes buffer b for call k + 2 has passed the barrier of call k + 1, which every wave reaches
// only after its reads of call k.
template <class Op>
__device__ __forceinline__ double lb_reduce(double v, double* red, int& flip, Op op) {
    v = group_reduce<64>(v, op);
    double* r = red + flip * LB_WAVES;
    flip ^= 1;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = r[0];
#pragma unroll
    for (int w = 1; w < LB_WAVES; ++w) s = op(s, r[w]);
    return s;
}

}  // namespace

__global__ void __launch_bounds__(LB_THREADS) k_lbfgs_direction(LbfgsArgs a) {
    __shared__ double red[2 * LB_WAVES];
    __shared__ double s_al[HPV_LBFGS_MAX_HISTORY];
    const int P = a.P, m = a.m, tid = threadIdx.x;
    const int head = a.ring[0];
    int n = a.ring[1];
    n = n < 0 ? 0 : (n > m ? m : n);
    const double* __restrict__ g = a.g;
    double* __restrict__ q = a.d;
    int flip = 0;
    // q = -g, with the partial sums of s_newest . q
    const double* __restrict__ Sn = n > 0 ? a.S + (long)((head + n - 1) % m) * P : nullptr;
    double part = 0.0;
    for (int i = tid; i < P; i += LB_THREADS) {
        const double v = -g[i];
        q[i] = v;
        if (Sn) part += Sn[i] * v;
    }
    // first loop, newest to oldest: al_k = rho_k s_k . q;  q -= al_k y_k
    for (int k = n - 1; k >= 0; --k) {
        const int slot = (head + k) % m;
        const double al = lb_reduce(part, red, flip, LbSum()) * a.rho[slot];
        if (tid == 0) s_al[k] = al;
        const double* __restrict__ Yk = a.Y + (long)slot * P;
        const double* __restrict__ Sm = k > 0 ? a.S + (long)((head + k - 1) % m) * P : nullptr;
        part = 0.0;
        for (int i = tid; i < P; i += LB_THREADS) {
            const double v = q[i] - al * Yk[i];
            q[i] = v;
            if (Sm) part += Sm[i] * v;
        }
    }
    // r = H_diag q, with the partial sums of y_oldest . r
    const double hd = *a.h_diag;
    {
        const double* __restrict__ Y0 = n > 0 ? a.Y + (long)(head % m) * P : nullptr;
        part = 0.0;
        for (int i = tid; i < P; i += LB_THREADS) {
            const double v = q[i] * hd;
            q[i] = v;
            if (Y0) part += Y0[i] * v;
        }
    }
    __syncthreads();      // s_al of thread 0 (n > 0: the reductions above have ordered all but the last store)
    // second loop, oldest to newest: be_k = rho_k y_k . r;  r += (al_k - be_k) s_k
    for (int k = 0; k < n; ++k) {
        const int slot = (head + k) % m;
        const double be = lb_reduce(part, red, flip, LbSum()) * a.rho[slot];
        const double c = s_al[k] - be;
        const double* __restrict__ Sk = a.S + (long)slot * P;
        const double* __restrict__ Yn = k + 1 < n ? a.Y + (long)((head + k + 1) % m) * P : nullptr;
        part = 0.0;
        for (int i = tid; i < P; i += LB_THREADS) {
            const double v = q[i] + c * Sk[i];
            q[i] = v;
            if (Yn) part += Yn[i] * v;
        }
    }
    // g . d, max|g|, sum|g|, max|d|
    double gd = 0.0, gmax = 0.0, gsum = 0.0, dmax = 0.0;
    for (int i = tid; i < P; i += LB_THREADS) {
        const double gi = g[i], di = q[i];
        gd += gi * di;
        gmax = fmax(gmax, fabs(gi));
        gsum += fabs(gi);
        dmax = fmax(dmax, fabs(di));
    }
    gd = lb_reduce(gd, red, flip, LbSum());
    gmax = lb_reduce(gmax, red, flip, LbMax());
    gsum = lb_reduce(gsum, red, flip, LbSum());
    dmax = lb_reduce(dmax, red, flip, LbMax());
    if (tid == 0) { a.scal[0] = gd; a.scal[1] = gmax; a.scal[2] = gsum; a.scal[3] = dmax; }
}

__global__ void __launch_bounds__(256) k_lbfgs_trial(const double* __restrict__ theta0, const double* __restrict__ d, double t,
                                                     double* __restrict__ theta, int P) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (long)gridDim.x * blockDim.x)
        theta[i] = theta0[i] + t * d[i];
}

__global__ void __launch_bounds__(LB_THREADS) k_lbfgs_probe(LbfgsArgs a, const double* __restrict__ RB, double* __restrict__ g_keep,
                                                            int with_d) {
    __shared__ double red[2 * LB_WAVES];
    const int P = a.P, tid = threadIdx.x;
    const double* __restrict__ d = a.d;
    int flip = 0;
    double gd = 0.0, gmax = 0.0;
    for (int i = tid; i < P; i += LB_THREADS) {
        const double gi = RB[i];
        g_keep[i] = gi;
        if (with_d) gd += gi * d[i];
        gmax = fmax(gmax, fabs(gi));
    }
    gd = lb_reduce(gd, red, flip, LbSum());
    gmax = lb_reduce(gmax, red, flip, LbMax());
    if (tid == 0) { a.scal[4] = RB[P] + RB[P + 1]; a.scal[5] = gd; a.scal[6] = gmax; a.scal[7] = 0.0; }
}

__global__ void __launch_bounds__(LB_THREADS) k_lbfgs_push(LbfgsArgs a, double t, const double* __restrict__ g_new) {
    __shared__ double red[2 * LB_WAVES];
    const int P = a.P, m = a.m, tid = threadIdx.x;
    const double* __restrict__ d = a.d;
    double* __restrict__ g = a.g;
    int flip = 0;
    double ys = 0.0, yy = 0.0;
    for (int i = tid; i < P; i += LB_THREADS) {
        const double y = g_new[i] - g[i], s = d[i] * t;
        ys += y * s;
        yy += y * y;
    }
    ys = lb_reduce(ys, red, flip, LbSum());
    yy = lb_reduce(yy, red, flip, LbSum());
    const int head = a.ring[0], n = a.ring[1];
    const bool keep = ys > HPV_LBFGS_YS_MIN;      // (false for a NaN as well)
    // a full ring drops its oldest pair: the new one takes that slot and the head moves on
    const int slot = n < m ? (head + n) % m : head;
    double* __restrict__ Sk = a.S + (long)slot * P;
    double* __restrict__ Yk = a.Y + (long)slot * P;
    for (int i = tid; i < P; i += LB_THREADS) {
        const double gn = g_new[i];
        if (keep) { Sk[i] = d[i] * t; Yk[i] = gn - g[i]; }
        g[i] = gn;
        a.theta0[i] = a.theta[i];
    }
    __syncthreads();      // every thread has read the ring's counters
    if (tid == 0) {
        if (keep) {
            a.rho[slot] = 1.0 / ys;
            *a.h_diag = ys / yy;
            if (n < m) a.ring[1] = n + 1; else a.ring[0] = (head + 1) % m;
        } else {
            a.ring[2] += 1;
        }
    }
}

void launch_lbfgs_direction(const LbfgsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_direction, dim3(1), dim3(LB_THREADS), 0, s, a);
}

void launch_lbfgs_trial(const LbfgsArgs& a, double t, hipStream_t s) {
    int b = (a.P + 255) / 256;
    hipLaunchKernelGGL(k_lbfgs_trial, dim3(b < 1 ? 1 : (b > 256 ? 256 : b)), dim3(256), 0, s, a.theta0, a.d, t, a.theta, a.P);
}

void launch_lbfgs_probe(const LbfgsArgs& a, const double* RB, double* g_keep, int with_d, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_probe, dim3(1), dim3(LB_THREADS), 0, s, a, RB, g_keep, with_d);
}

void launch_lbfgs_push(const LbfgsArgs& a, double t, const double* g_new, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_push, dim3(1), dim3(LB_THREADS), 0, s, a, t, g_new);
}
