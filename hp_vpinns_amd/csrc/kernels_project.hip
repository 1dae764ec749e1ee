// Tensor-product projection kernel for the hot element shapes: one wavefront per element,
// test-function tables staged once per workgroup in LDS, sum-factorised contractions
// (x then y), wave-level synchronisation only, shuffle reductions for the element loss.
//
//   forward :  T_t[j][r] = sum_i AX_t[r][i] G_t[j][i]            AX = w_x * phi^(dx)      (P2:94-105)
//              U[k][r]  += m_t c_t sum_j BY_t[k][j] T_t[j][r]    BY = w_y * phi^(dy)
//              R = U - F,  loss_e = mean(R^2)                                             (P2:118-119)
//   adjoint :  S_t[k][i] = sum_r AX_t[r][i] (2/NR) R[k][r]
//              Ghat_t[j][i] = c_t sum_k BY_t[k][j] S_t[k][i],   GBAR[ch] = sum_t alpha_t[ch] m_t Ghat_t
//
// HBM traffic per element = read the integrated channels + F, write the adjoint channels + R (channels no
// term uses are neither read nor written; their GBAR rows are zeroed once by the host).  This is the kernel
// judged against the HBM roofline on the scaled synthetic batch.
#include <algorithm>

#include "hpv_internal.h"
#include "hpv_project_wg.h"


// Work decomposition: "a lane owns a line".  LPE = max(QX,QY) lanes serve one element, EPW = 64/LPE elements
// share a wavefront (3 for 20x20 points, 6 for 10x10).  In every contraction the lane keeps its line of
// element data in registers and the test-function table entry is WAVE-UNIFORM (same index for all lanes
// at the same instruction): tables are staged once per workgroup in LDS and read with broadcast reads.
// The y-contraction comes first with the lane owning COLUMN i of the integrand (all j): those loads are
// coalesced straight from HBM into registers (q = j*QX + i, i fastest), so no LDS staging of the
// integrand is needed; one small LDS transpose (NTY x QX per element) separates the two contractions,
// in the forward and again in the adjoint.  Residual rows stay in registers between forward and adjoint.
//   forward :  T[k][i]  = sum_j BY[k][j] G[j][i]      (lane = i)     ->LDS->
//              U[k][r] += m c sum_i AX[r][i] T[k][i]   (lane = k)
//   adjoint :  V[k][i]  = sum_r AX[r][i] Rs[k][r]      (lane = k)     ->LDS->
//              Gh[j][i] = c sum_k BY[k][j] V[k][i]     (lane = i)     -> coalesced stores
// The one-hot streaming instantiation: 8 waves per workgroup, 4 waves per SIMD (126 VGPRs), a term's channel column loaded when the
// term starts.  (Requesting the NEXT column while this one's contractions run measured slower: profiles/r04_notes.md)
// (Writing R of the one-hot instantiation with a non-temporal hint measured no gain and +5 % written bytes: profiles/r04_notes.md.)
// k_project_tp reads its test-function tables from global memory at wave-uniform addresses -- scalar loads, an SGPR operand per
// FMA -- instead of LDS broadcast reads (800 ds_read per element group with an s_waitcnt in front of the FMAs that use them; the
// LDS-table form lost: profiles/r04_notes.md section 1).
__device__ __forceinline__ void pj_stream_store(double* p, double v) {
    *p = v;
}

struct ActiveCh {
    int n;                      // number of channels some term integrates
    int id[HPV_MAXC];           // their channel indices
};

// OH ("one-hot"): term t integrates exactly the active channel t and nothing else (Poisson-2D var_form 1: u_x, u_y).
// The integrand column then IS the prefetched channel column (alpha folds into the term coefficient) and the
// adjoint column of term t is stored straight to channel t -- no gcol / gacc copies.  With 8 waves per workgroup the
// channel column of a term is loaded when the term starts (124 VGPRs, 4 waves per SIMD, 2 x 63.6 KB LDS per CU):
// measured 3.6 TB/s against 3.15 TB/s for the 202-VGPR / 2-waves-per-SIMD general variant on the 2^18-element batch
// (5 waves per SIMD spills: 2.5 TB/s).
template <int QX, int QY, int NTX, int NTY, int NA, bool EPS, int PJ_WAVES, bool OH = false>
__global__ void __launch_bounds__(PJ_WAVES * 64, (OH && PJ_WAVES == 8) ? 4 : 1) k_project_tp(ProjDesc pd, ActiveCh ac, const double* __restrict__ OUT,
                                                        double* __restrict__ GBAR, double* __restrict__ R,
                                                        const double* __restrict__ F, const double* __restrict__ coef,
                                                        long coef_stride, const double* __restrict__ wtx,
                                                        const double* __restrict__ wty, const double* __restrict__ eps_ptr,
                                                        double* __restrict__ loss_e, double* __restrict__ deps_e, long N,
                                                        long n_elem, int do_adjoint) {
    constexpr int NQ = QX * QY, NR = NTX * NTY;
    constexpr int LPE = QX > QY ? QX : QY;
    static_assert(NTX <= LPE && NTY <= LPE && LPE <= 64, "element shape");
    constexpr int EPW = 64 / LPE;
    constexpr int LDT = QX + 1;
    constexpr int TB_D = EPW * NTY * LDT;
    constexpr int WAVE_DOUBLES = TB_D + 64;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // (the tables are SGPR operands: nothing is staged, the kernel starts with its first element group's loads.  The launch still
    //  reserves the room of the LDS-table form in front of the wave tiles: both tables in both orientations.)
    double* Tb = sm + 2 * (3 * NTX * QX + 3 * NTY * QY) + wv * WAVE_DOUBLES;   // [EPW][NTY][LDT]  transpose tile (T, then V)
    double* Rd = Tb + TB_D;                                // [64] slot-wise reductions
    const int slot = lane / LPE, li = lane % LPE;
    const bool lane_ok = slot < EPW;

    const int nterms = pd.nterms;
    const double eps = eps_ptr ? eps_ptr[0] : 0.0;
    const double sc = 2.0 / (double)NR;

    const long ngroups = (n_elem + EPW - 1) / EPW;
    constexpr bool LATE = OH && PJ_WAVES == 8;   // 4 waves/SIMD (124 VGPRs): the other waves hide the per-term round trip

    const long gstride = (long)gridDim.x * PJ_WAVES;
    for (long grp = (long)blockIdx.x * PJ_WAVES + wv; grp < ngroups; grp += gstride) {
        const long e = grp * EPW + slot;
        const bool ev = lane_ok && e < n_elem;
        const bool col = ev && li < QX;     // this lane owns quadrature column i = li
        const bool row = ev && li < NTY;    // this lane owns residual row k = li
        const double* __restrict__ Oe = OUT + e * NQ + li;
        // all HBM reads of the group are issued up front (one memory round trip): the right-hand-side row
        // and the quadrature column of every integrated channel
        double u[NTX];
#pragma unroll
        for (int r = 0; r < NTX; ++r) u[r] = (row && F) ? -F[e * NR + li * NTX + r] : 0.0;
        // the term coefficients are requested HERE, ahead of any prefetch of the next column: vector loads return in order, and a
        // wait for a coefficient issued behind the prefetch (s_waitcnt vmcnt(0)) would wait for the prefetch as well
        double cf[OH ? NA : HPV_MAXT];
#pragma unroll
        for (int t = 0; t < (OH ? NA : HPV_MAXT); ++t) cf[t] = (ev && (OH || t < nterms)) ? coef[(long)t * coef_stride + e] : 0.0;
        double o[NA][QY];
        if constexpr (!LATE) {
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int j = 0; j < QY; ++j) o[a][j] = col ? Oe[(long)ac.id[a] * N + j * QX] : 0.0;
        }
        double gacc[OH ? 1 : NA][OH ? 1 : QY];
        if constexpr (!OH) {
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int j = 0; j < QY; ++j) gacc[a][j] = 0.0;
        }

#pragma unroll
        for (int t = 0; t < (OH ? NA : HPV_MAXT); ++t) {
            if (!OH && t >= nterms) break;
            const TermDesc& td = pd.t[t];
            // (a) integrand column of this term from the prefetched channels
            double gcol[QY];
            double alpha_t = 1.0;
            if constexpr (OH) {
                alpha_t = td.a0[ac.id[t]] + eps * td.a1[ac.id[t]];
                if constexpr (LATE) {
#pragma unroll
                    for (int j = 0; j < QY; ++j) gcol[j] = col ? Oe[(long)ac.id[t] * N + j * QX] : 0.0;
                } else {
#pragma unroll
                    for (int j = 0; j < QY; ++j) gcol[j] = o[t][j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < QY; ++j) gcol[j] = 0.0;
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const double al = td.a0[ac.id[a]] + eps * td.a1[ac.id[a]];
#pragma unroll
                    for (int j = 0; j < QY; ++j) gcol[j] = fma(al, o[a][j], gcol[j]);
                }
            }
            pj_wave_sync();   // previous readers of Tb are done
            // (b) y-contraction, lane = column i
            if (col) {
                const double* __restrict__ byg = wty + (long)td.dy * (NTY * QY);      // [k][j], wave-uniform
                double acc[NTY];
#pragma unroll
                for (int k = 0; k < NTY; ++k) acc[k] = 0.0;
#pragma unroll
                for (int k = 0; k < NTY; ++k)
#pragma unroll
                    for (int j = 0; j < QY; ++j) acc[k] = fma(byg[k * QY + j], gcol[j], acc[k]);
#pragma unroll
                for (int k = 0; k < NTY; ++k) Tb[slot * (NTY * LDT) + k * LDT + li] = acc[k];
            }
            pj_wave_sync();
            // (c) x-contraction, lane = residual row k
            if (row) {
                const double* __restrict__ axg = wtx + (long)td.dx * (NTX * QX);      // [r][i], wave-uniform
                const double c = cf[t] * (td.eps_mult ? eps : 1.0) * alpha_t;
                double trow[QX], acc[NTX];
#pragma unroll
                for (int i = 0; i < QX; ++i) trow[i] = Tb[slot * (NTY * LDT) + li * LDT + i];
#pragma unroll
                for (int r = 0; r < NTX; ++r) acc[r] = 0.0;
#pragma unroll
                for (int r = 0; r < NTX; ++r)
#pragma unroll
                    for (int i = 0; i < QX; ++i) acc[r] = fma(axg[r * QX + i], trow[i], acc[r]);
#pragma unroll
                for (int r = 0; r < NTX; ++r) u[r] = fma(c, acc[r], u[r]);
            }
        }
        // residual row, element loss
        double sq = 0.0;
        if (row) {
#pragma unroll
            for (int r = 0; r < NTX; ++r) {
                if constexpr (OH) pj_stream_store(R + e * NR + li * NTX + r, u[r]); else R[e * NR + li * NTX + r] = u[r];
                sq = fma(u[r], u[r], sq);
                u[r] *= sc;
            }
        }
        Rd[lane] = sq;
        pj_wave_sync();
        if (ev && li == 0) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NTY; ++k) s += Rd[slot * LPE + k];
            loss_e[e] = s / (double)NR;
        }
        if (!do_adjoint) continue;

        double deps = 0.0;
#pragma unroll
        for (int t = 0; t < (OH ? NA : HPV_MAXT); ++t) {
            if (!OH && t >= nterms) break;
            const TermDesc& td = pd.t[t];
            pj_wave_sync();
            // (d) V[k][i] = sum_r AX[r][i] Rs[k][r], lane = row k
            if (row) {
                const double* ax = wtx + (long)td.dx * (NTX * QX);
                double acc[QX];
#pragma unroll
                for (int i = 0; i < QX; ++i) acc[i] = 0.0;
#pragma unroll
                for (int r = 0; r < NTX; ++r)
#pragma unroll
                    for (int i = 0; i < QX; ++i) acc[i] = fma(ax[r * QX + i], u[r], acc[i]);
#pragma unroll
                for (int i = 0; i < QX; ++i) Tb[slot * (NTY * LDT) + li * LDT + i] = acc[i];
            }
            pj_wave_sync();
            // (e) Gh[j][i] = c sum_k BY[k][j] V[k][i], lane = column i; scattered onto the integrated channels
            if (col) {
                const double* by = wty + (long)td.dy * (NTY * QY);
                const double c = cf[t];
                const double m = td.eps_mult ? eps : 1.0;
                double vcol[NTY], gh[QY];
#pragma unroll
                for (int k = 0; k < NTY; ++k) vcol[k] = Tb[slot * (NTY * LDT) + k * LDT + li];
#pragma unroll
                for (int j = 0; j < QY; ++j) gh[j] = 0.0;
#pragma unroll
                for (int k = 0; k < NTY; ++k)
#pragma unroll
                    for (int j = 0; j < QY; ++j) gh[j] = fma(by[k * QY + j], vcol[k], gh[j]);
                if constexpr (OH) {   // term t <-> channel t: its adjoint column goes out directly, coalesced
                    const double al = (td.a0[ac.id[t]] + eps * td.a1[ac.id[t]]) * (m * c);
                    double* __restrict__ Ge = GBAR + e * NQ + li + (long)ac.id[t] * N;
#pragma unroll
                    for (int j = 0; j < QY; ++j) Ge[j * QX] = al * gh[j];
                } else {
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        const double al = (td.a0[ac.id[a]] + eps * td.a1[ac.id[a]]) * (m * c);
#pragma unroll
                        for (int j = 0; j < QY; ++j) gacc[a][j] = fma(al, gh[j], gacc[a][j]);
                    }
                }
                if constexpr (EPS) {   // d loss / d epsilon (P3:63): through alpha(eps) and eps-multiplied terms
#pragma unroll
                    for (int j = 0; j < QY; ++j) {
                        double g1 = 0.0, gt = 0.0;
#pragma unroll
                        for (int a = 0; a < NA; ++a) {
                            g1 = fma(td.a1[ac.id[a]], o[a][j], g1);
                            gt = fma(td.a0[ac.id[a]] + eps * td.a1[ac.id[a]], o[a][j], gt);
                        }
                        deps = fma(c * gh[j], m * g1 + (td.eps_mult ? gt : 0.0), deps);
                    }
                }
            }
        }
        // (f) adjoint of the integrated channels, coalesced (channels no term uses are never touched)
        if (!OH && col) {
            double* __restrict__ Ge = GBAR + e * NQ + li;
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int j = 0; j < QY; ++j) Ge[(long)ac.id[a] * N + j * QX] = gacc[a][j];
        }
        if constexpr (EPS) {
            pj_wave_sync();
            Rd[lane] = deps;
            pj_wave_sync();
            if (ev && li == 0) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < QX; ++i) s += Rd[slot * LPE + i];
                deps_e[e] = s;
            }
        }
    }
}

template <int QX, int QY, int NTX, int NTY, int NA, bool EPS, int PJ_WAVES, bool OH = false>
static void launch_tp3(const ProjArgs& pa, const ActiveCh& ac, long n_elem, long ngroups, hipStream_t s) {
    constexpr int LPE = QX > QY ? QX : QY;
    constexpr int EPW = 64 / LPE;
    constexpr int WAVE_DOUBLES = EPW * NTY * (QX + 1) + 64;
    constexpr size_t lds = (size_t)(2 * (3 * NTX * QX + 3 * NTY * QY) + PJ_WAVES * WAVE_DOUBLES) * sizeof(double);
    long blocks = (ngroups + PJ_WAVES - 1) / PJ_WAVES;
    // (scripts/hbm_read_probe.hip: a plain read stream is FASTER with fewer waves in flight -- 6.3-6.6 TB/s at 2 workgroups per CU against 5.0-5.5 at 4-8)
    if (blocks > 256 * 16) blocks = 256 * 16;   // grid-stride beyond that
    if (lds > 65536) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute((const void*)k_project_tp<QX, QY, NTX, NTY, NA, EPS, PJ_WAVES, OH>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr_set = true;
        }
    }
    hipLaunchKernelGGL((k_project_tp<QX, QY, NTX, NTY, NA, EPS, PJ_WAVES, OH>), dim3((unsigned)blocks), dim3(PJ_WAVES * 64), lds, s,
                       pa.pd, ac, pa.OUT, pa.GBAR, pa.R, pa.F, pa.coef, pa.coef_stride, pa.wtx, pa.wty, pa.eps_ptr, pa.loss_e, pa.deps_e, pa.N, n_elem,
                       pa.do_adjoint);
}

template <int QX, int QY, int NTX, int NTY, int NA, bool EPS>
static bool launch_tp2(const ProjArgs& pa, const ActiveCh& ac, long n_elem, hipStream_t s) {
    const ProjDesc& pd = pa.pd;
    constexpr int LPE = QX > QY ? QX : QY;
    constexpr int EPW = 64 / LPE;
    const long ngroups = (n_elem + EPW - 1) / EPW;
    // few element groups (config-4 scale): one wavefront per workgroup spreads the groups over as many CUs as
    // possible (each wave then has a CU's LDS port to itself for its ~800 broadcast table reads); large batches:
    // four waves per workgroup amortise the table staging
    // one-hot term/channel structure (see k_project_tp): term t integrates active channel t only
    bool onehot = !EPS && pd.nterms == NA && NA >= 2;
    for (int t = 0; t < pd.nterms && onehot; ++t)
        for (int a = 0; a < NA; ++a)
            if (a != t && (pd.t[t].a0[ac.id[a]] != 0.0 || pd.t[t].a1[ac.id[a]] != 0.0)) onehot = false;
#define HPV_GO(W_, OH_) launch_tp3<QX, QY, NTX, NTY, NA, EPS, W_, OH_>(pa, ac, n_elem, ngroups, s)
    if constexpr (!EPS && NA >= 2) {
        if (onehot) {
            if (ngroups <= 1024) HPV_GO(1, true); else HPV_GO(8, true);
            return true;
        }
    }
    if (ngroups <= 1024) HPV_GO(1, false); else HPV_GO(4, false);
#undef HPV_GO
    return true;
}

template <int QX, int QY, int NTX, int NTY>
static bool launch_tp(const ProjArgs& pa, long n_elem, hipStream_t s) {
    const ProjDesc& pd = pa.pd;
    ActiveCh ac{};
    for (int ch = 0; ch < pd.C; ++ch) {
        bool used = false;
        for (int t = 0; t < pd.nterms; ++t) used |= (pd.t[t].a0[ch] != 0.0 || pd.t[t].a1[ch] != 0.0);
        if (used) ac.id[ac.n++] = ch;
    }
#define HPV_NA(NA_, EPS_)                                                                                              \
    if (ac.n == NA_ && (pd.has_eps != 0) == EPS_)                                                                      \
        return launch_tp2<QX, QY, NTX, NTY, NA_, EPS_>(pa, ac, n_elem, s);
    HPV_NA(1, false) HPV_NA(2, false) HPV_NA(2, true) HPV_NA(3, true)
#undef HPV_NA
    return false;
}

// ------------------------------------------------------------------------------------------------
// Workgroup-per-element variant for TALL elements (80 points per direction: the 1-D rule of P1:238 and the
// AdvDiff 80x80 rule of BASELINE config 5), where a line of the element no longer fits the lanes of one wave.
// Same sum-factorised algorithm as k_project (x-contraction, then y), but with compile-time shapes, the
// term's two tables staged in LDS, the integrand staged once in LDS from batched coalesced loads, and the
// Poisson-1D element-edge term (P1:90) supported.
// ------------------------------------------------------------------------------------------------
#define PW_BLOCK 1024
template <int QX, int QY, int NTX, int NTY>
__global__ void __launch_bounds__(PW_BLOCK) k_project_wg(ProjArgs pa) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    project_element_wg<QX, QY, NTX, NTY, PW_BLOCK>(pa, (long)blockIdx.x, sm);
}

template <int QX, int QY, int NTX, int NTY>
static bool launch_wg(const ProjArgs& pa, long n_elem, hipStream_t s) {
    constexpr size_t lds = (size_t)project_wg_lds_doubles<QX, QY, NTX, NTY>() * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {   // > 64 KB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute((const void*)k_project_wg<QX, QY, NTX, NTY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((k_project_wg<QX, QY, NTX, NTY>), dim3((unsigned)n_elem), dim3(PW_BLOCK), lds, s, pa);
    return true;
}

// Workgroups per element of the row-split projection (1: not applicable); loss_e / deps_e then hold n_elem * split entries.
int project_row_split(const ProjDesc& pd, long n_elem, int backend_generic) {
    if (backend_generic || pd.edge || n_elem <= 0 || n_elem * PJ_SPLIT > 4096) return 1;
    if (pd.qx == 80 && pd.qy == 80 && pd.ntx == 5 && pd.nty == 5) return PJ_SPLIT;
    return 1;
}

template <int QX, int QY, int NTX, int NTY>
static void launch_rows(const ProjArgs& pa, long n_elem, double* upart, hipStream_t s) {
    constexpr size_t lds = (size_t)project_rows_lds_doubles<QX, QY, NTX, NTY>() * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)k_project_rows_fwd<QX, QY, NTX, NTY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void*)k_project_rows_adj<QX, QY, NTX, NTY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    const unsigned blocks = (unsigned)(n_elem * PJ_SPLIT);
    hipLaunchKernelGGL((k_project_rows_fwd<QX, QY, NTX, NTY>), dim3(blocks), dim3(PJ_RBLOCK), lds, s, pa, upart);
    hipLaunchKernelGGL((k_project_rows_adj<QX, QY, NTX, NTY>), dim3(blocks), dim3(PJ_RBLOCK), lds, s, pa, upart);
}

bool launch_project_wg(const ProjArgs& pa, long n_elem, hipStream_t s, double* upart) {
    const ProjDesc& pd = pa.pd;
    if (n_elem <= 0) return false;
    if (upart && !pd.nact && project_row_split(pd, n_elem, 0) > 1) {   // few tall elements: PJ_SPLIT workgroups per element, two phases
        ProjArgs rows = pa;      // (the row-split kernels take no element-edge term)
        rows.edge_u = rows.edge_dphi = rows.edge_coef = nullptr; rows.edge_gbar = nullptr;
        launch_rows<80, 80, 5, 5>(rows, n_elem, upart, s);
        return true;
    }
#define HPV_WG(QX_, QY_, NTX_, NTY_, EXACT_)                                                                              \
    if (pd.qx == QX_ && pd.qy == QY_ && (EXACT_ ? pd.ntx == NTX_ && pd.nty == NTY_ : pd.ntx >= 1 && pd.ntx <= NTX_ && pd.nty >= 1 && pd.nty <= NTY_))   \
        return launch_wg<QX_, QY_, NTX_, NTY_>(pa, n_elem, s);
    HPV_WG(80, 1, 60, 1, true)     // Poisson-1D reference rule: N_Quad = 80, N_testfcn = 60 (P1:237-238; BASELINE configs 1, 2)
    HPV_WG(80, 80, 5, 5, true)     // AdvDiff with the 80-point rule per direction (BASELINE config 5)
    // small grids of the 2-D shapes (round 4): one 1024-thread workgroup per element spreads a few hundred elements over all CUs,
    // where "a lane owns a line" (k_project_tp: 3-6 elements per WAVE) leaves most of the chip idle -- the caller prefers this
    // launch when the shard has at most two elements per CU
    // (these take any smaller test-function counts at run time: project_element_wg stages the missing functions' tables as zeros)
    HPV_WG(20, 20, 10, 10, false)
    HPV_WG(10, 10, 5, 5, false)
    HPV_WG(16, 16, 8, 8, false)
    HPV_WG(12, 12, 6, 6, false)
    // larger rules (no whole-iteration kernel takes them: forward -> this -> reverse): 35 -> ~10 us of a 120 us iteration at 24x24 points
    HPV_WG(24, 24, 12, 12, false)
    HPV_WG(28, 28, 14, 14, false)
    HPV_WG(32, 32, 16, 16, false)
    HPV_WG(36, 36, 18, 18, false)
    HPV_WG(40, 40, 20, 20, false)
#undef HPV_WG
    return false;
}

// Returns false when the element shape has no specialised instantiation (caller falls back to k_project).
bool launch_project_tp(const ProjArgs& pa, long n_elem, hipStream_t s) {
    const ProjDesc& pd = pa.pd;
    if (pd.nact) return false;   // per-element active test counts: the general projections only
    if (pd.edge || n_elem <= 0) return false;
#define HPV_TP(QX_, QY_, NTX_, NTY_)                                                                              \
    if (pd.qx == QX_ && pd.qy == QY_ && pd.ntx == NTX_ && pd.nty == NTY_)                                          \
        return launch_tp<QX_, QY_, NTX_, NTY_>(pa, n_elem, s);
    HPV_TP(20, 20, 10, 10)   // BASELINE config 4
    HPV_TP(10, 10, 5, 5)     // BASELINE config 3, the Poisson-2D and AdvDiff reference defaults (P2:282-286, P3:47-51)
#undef HPV_TP
    return false;
}
