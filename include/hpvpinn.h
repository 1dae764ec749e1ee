/* hpvpinn.h -- C-ABI of libhpvpinn.so, the MI355X (gfx950) hp-VPINN training path.
 *
 * The reference (ehsankharazmi/hp-VPINNs) has no FFI / plugin interface: its boundary is the
 * Python `class VPINN` of each driver script.  This header is the plain-C surface a binding of
 * that class needs -- opaque handle, plain pointers and sizes, status codes; no torch types.
 * Every entry point cites the reference lines whose work it replaces
 * (P1 = main/Poisson-1D/hp-VPINN-Poisson-1D.py, P2 = main/Poisson-2D/hp-VPINN-Poisson-2D.py,
 *  P3 = main/AdvDiff-Identification/hp-VPINN-AdvDiff-Identification.py).
 *
 * Conventions
 *   - all floating point data is IEEE double (the reference is tf.float64 throughout);
 *   - the caller owns every host buffer; the library copies on set_* and owns all device memory;
 *   - return 0 = OK, negative = error (message via hpv_last_error); nothing is thread-safe per
 *     handle, independent handles may live on different threads / processes (one per GPU);
 *   - parameter packing: theta = [W0, b0, W1, b1, ..., (epsilon)], W_l row-major [in, out]
 *     (row-vector convention H @ W + b of P1:128-138), epsilon only for HPV_PDE_ADVDIFF;
 *   - element index e = ex * ney + ey (P2:69-70 loop order; F_ext_total[ex, ey] at P2:414);
 *     quadrature index inside an element q = j * qx + i, x fastest (P2:362-365);
 *   - residual entries of one element are [k (y / t index)][r (x index)] (P2:94-96).
 */
#ifndef HPVPINN_H
#define HPVPINN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPV_MAX_LAYERS 16

enum { HPV_PDE_POISSON1D = 0, HPV_PDE_POISSON2D = 1, HPV_PDE_ADVDIFF = 2,
       HPV_PDE_LINEAR1D = 3, HPV_PDE_LINEAR2D = 4 };   /* variable-coefficient linear problems: hpv_set_operator */
enum { HPV_ACT_TANH = 0, HPV_ACT_SIN = 1 };
enum { HPV_BACKEND_AUTO = 0, HPV_BACKEND_GENERIC = 1, HPV_BACKEND_MFMA = 2 };
enum { HPV_SCHEME_VPINN = 0, HPV_SCHEME_PINN = 1 };

typedef struct hpv_ctx* hpv_handle;

typedef struct hpv_config {
    int pde;                      /* HPV_PDE_*                                                        */
    int var_form;                 /* P1:82-91 (1,2,3) / P2:93-115 (0,1,2) / P3:161-174 (0,1)           */
    int act;                      /* HPV_ACT_SIN for P1:134, HPV_ACT_TANH for P2:165, P3:226          */
    int n_layers;                 /* len(layers), e.g. 5 for [2,20,20,20,1]                           */
    int layers[HPV_MAX_LAYERS];
    double lr, beta1, beta2, eps; /* tf.train.AdamOptimizer(LR) defaults: 1e-3, 0.9, 0.999, 1e-8     */
    double lossb_weight;          /* P1:100 (1), P2:127 (10), P3:184 (10)                             */
    double V;                     /* advection speed, P3:43                                           */
    int device;                   /* HIP device ordinal                                               */
    int backend;                  /* HPV_BACKEND_*                                                    */
    int scheme;                   /* HPV_SCHEME_VPINN (default) or HPV_SCHEME_PINN (P2:126-129; every pde) */
} hpv_config;

/* Construction = the graph-build part of VPINN.__init__ (P1:31-107, P2:28-136, P3:60-197). */
int hpv_create(hpv_handle* out, const hpv_config* cfg);
void hpv_destroy(hpv_handle h);
const char* hpv_last_error(hpv_handle h); /* h may be NULL: last create() error */

/* Run every kernel of this handle on an existing HIP stream (hipStream_t passed as void*), e.g.
 * torch's current stream so that a torch.distributed collective orders after the kernels. */
int hpv_set_stream(hpv_handle h, void* hip_stream);

/* 1-D reference quadrature rule per direction: nodes xi in [-1,1] and weights (P1:312-316,
 * P2:355-360, P3:395-400).  qy = 1 (and yi = wy = NULL) for the 1-D problem. */
int hpv_set_quadrature(hpv_handle h, const double* xi, const double* wx, int qx,
                       const double* yi, const double* wy, int qy);

/* Test-function tables phi, phi', phi'' at the reference nodes, each [ntest][q] row-major
 * (values of VPINN.Test_fcn / dTest_fcn, P1:157-183).  nty = 1, tables NULL in 1-D.
 * edge_dphi = phi'_k(-1), phi'_k(+1) as [ntx][2], needed only by Poisson-1D var_form 3 (P1:79,90). */
int hpv_set_tables(hpv_handle h, const double* phix, const double* dphix, const double* d2phix, int ntx,
                   const double* phiy, const double* dphiy, const double* d2phiy, int nty,
                   const double* edge_dphi);

/* Element grids (P1:264-273, P2:370-376, P3:404-410) and the slice [e_begin, e_end) of flattened
 * elements this handle (this GPU) owns -- the data-parallel shard.  The affine map of the
 * reference nodes into each element (P1:69, P2:75-76, P3:120-121) is evaluated here. */
int hpv_set_elements(hpv_handle h, const double* gridx, int nex, const double* gridy, int ney,
                     int e_begin, int e_end);

/* Elements as an arbitrary list of axis-parallel boxes instead of a tensor grid (local h-refinement): boxes is [n_total][2*dim]
 * row-major = (x0, x1) in 1-D, (x0, x1, y0, y1) in 2-D / (x0, x1, t0, t1) for AdvDiff; the element index e is the row of `boxes`
 * and [e_begin, e_end) slices the list as it slices a grid (multi-GPU sharding needs nothing else).  Same preconditions, return
 * codes and side effects as hpv_set_elements, which is this call on the boxes of e = ex*ney + ey: a box list made from a grid is
 * bit-identical to the grid.  Every per-element input (hpv_set_rhs, hpv_set_active_tests[_2d]) then counts n_total elements.
 * Each box is checked for finite bounds and x0 < x1 (y0 < y1).  The list is NOT checked for overlap or for covering the domain:
 * the test functions vanish on every element's boundary, elements are independent and hanging nodes are harmless, so any list
 * is a valid set of test spaces -- whether it is the intended one is the caller's business. */
int hpv_set_element_boxes(hpv_handle h, const double* boxes, int n_total, int e_begin, int e_end);

/* Right-hand sides F_ext_total for ALL elements of the mesh, C-order [n_total][nty][ntx] with n_total = nex*ney of a grid
 * (e = ex*ney + ey, i.e. [nex][ney][nty][ntx]: P1:294, P2:414) or the rows of a box list; pass NULL for a zero right-hand
 * side (P3:180). */
int hpv_set_rhs(hpv_handle h, const double* F, size_t n);

/* p-refinement of the 1-D driver: element e projects onto its first n_active[e] <= ntest test functions only and its loss
 * is the mean over those (P1:66-67: Ntest_element = len(F_ext_total[e]); the driver builds F_ext_total from the per-element
 * list N_testfcn_total, P1:268-281).  n = all elements of the mesh (nex of a grid, n_total of a box list); rows of F beyond n_active[e] are ignored and the
 * residuals returned for them are zero.  NULL restores "all ntest in every element".  1-D only: 2-D handles are refused
 * here and take their counts through hpv_set_active_tests_2d below. */
int hpv_set_active_tests(hpv_handle h, const int* n_active, int n);

/* p-refinement of the 2-D drivers (Poisson-2D, AdvDiff; variational scheme): the reference classes read the number of test
 * functions per element column and per element row -- Ntest_elementx = N_testfcn[0][ex], Ntest_elementy = N_testfcn[1][ey]
 * (P2:72-73, P3:112-113) -- build that element's tables from them (P2:85-88, P3:127-130) and take its reduce_mean over exactly
 * those residuals (P2:118-120).  Only the Poisson-2D DRIVER's np.reshape of F_ext_total (P2:414) asks for equal counts; the
 * AdvDiff right-hand side is zero (P3:180).
 * n = nex*ney of a grid, n_total of a box list: the counts of ALL elements of the mesh, indexed by the flattened element
 * e = ex*ney + ey (the row of the box list), 1 <= nax[e] <= ntx and
 * 1 <= nay[e] <= nty -- one PAIR per element, a superset of the reference's column x row product.  Element e projects onto its
 * first nax[e] x nay[e] test functions (the family is nested: the first rows of a larger table are the smaller table) and its
 * loss is the mean over those nax[e]*nay[e] residuals; rows and columns of F beyond the counts are ignored, the residuals
 * hpv_get_residuals returns for them are exactly 0 (layout [ne][nty][ntx] as ever).  The owned range [e_begin, e_end) is sliced
 * inside and the counts are re-applied after hpv_set_elements / hpv_set_tables.  NULL, NULL restores "all ntx x nty everywhere"
 * bit for bit.  Refused for 1-D handles, the strong-form PINN scheme, a wrong n and counts out of range. */
int hpv_set_active_tests_2d(hpv_handle h, const int* nax, const int* nay, int n);

/* Variable-coefficient convection-diffusion-reaction problems (an extension: HPV_PDE_LINEAR1D, HPV_PDE_LINEAR2D; no reference
 * counterpart).  With the sign convention that makes Poisson kx = ky = 1,
 *     L u = d/dx(kx u_x) + d/dy(ky u_y) + bx u_x + by u_y + s u = f            1-D:  (k u')' + b u' + s u = f
 * and kx, ky, bx, by, s given at the handle's quadrature points.  Every test function v_kr = phi_r(x) phi_k(y) vanishes on its
 * element's boundary, so the once-integrated-by-parts residual of element e is
 *     R[e][k][r] = -(J/Jx) sum_q w_q kx u_x phi_r' phi_k - (J/Jy) sum_q w_q ky u_y phi_r phi_k'
 *                  + J sum_q w_q (bx u_x + by u_y + s u) phi_r phi_k - F[e][k][r]
 * (J = Jx Jy; 1-D: no ky / by pieces, J = Jx; table derivatives with respect to the reference coordinate; F as hpv_assemble_rhs
 * builds it), lossv = sum_e mean over the ACTIVE test functions of R^2, loss = lossb_weight * lossb + lossf + lossv.
 * Special cases: k = 1, b = s = 0 is Poisson-2D var_form 1; kx = -eps, ky = 0, bx = V, by = 1 is AdvDiff var_form 1 at a fixed
 * epsilon; 1-D k = -1 is Poisson-1D var_form 2.
 * Such a handle is created with var_form = 1 and HPV_SCHEME_VPINN (anything else is refused), has no trainable coefficient unless
 * it is created with hpv_create_ex (below; hpv_num_params then counts them behind the network) and runs forward -> k_project_lin -> reverse (hpv_pass_structure 0).  Everything
 * else of the variational scheme works on it unchanged; the strong form needs derivatives of k and is refused:
 * hpv_set_collocation*, hpv_residual_points, hpv_element_indicators (negative status, the handle stays usable).  Refinement
 * indicators from the strong residual at the elements' own quadrature points are an opt-in: hpv_set_strong_form below.
 *
 * coef is [K][n_owned*qx*qy] in planes, K = 3 in 1-D in the order (k, b, s), K = 5 in 2-D in the order (kx, ky, bx, by, s); each
 * plane element-major over the OWNED elements, q = j*qx + i (the layout of f_quad in hpv_assemble_rhs); n = K*n_owned*qx*qy.
 * Everything is copied.  Waits for the handle's stream and drops the captured iteration graphs (like hpv_set_data).
 * hpv_set_elements / hpv_set_element_boxes invalidate the planes: a pass then answers -3 until they are set again.  The planes are
 * not state: hpv_get_state / hpv_set_state do not carry them.
 * Returns 0; -1 for a handle of another problem, a wrong n, NULL, a non-finite value; -3 before hpv_set_elements; -2 on a HIP error. */
int hpv_set_operator(hpv_handle h, const double* coef, size_t n);

/* A pointwise nonlinear term on a handle of the class above (HPV_PDE_LINEAR1D / _LINEAR2D).  With L u the operator of
 * hpv_set_operator and its sign convention unchanged,
 *     L u + N(x; u, grad u) = f
 *     N = a2 u^2 + a3 u^3 + ae exp(u) + u (gx u_x + gy u_y)                     1-D:  a2 u^2 + a3 u^3 + ae exp(u) + g u u_x
 * with a2, a3, ae, gx, gy given at the handle's quadrature points.  N is projected against phi_r phi_k without integration by
 * parts: it joins the integrand (bx u_x + by u_y + s u) of R above; tables, masking, F, lossv and the loss triple are unchanged,
 * and the gradient follows by the chain rule at the point (k_project_nl, csrc/kernels_nonlin.hip).
 * Special cases: space-time viscous Burgers u_t + u u_x - nu u_xx = 0 is kx = -nu, ky = 0, by = 1, gx = 1 on a 2-D handle with
 * y = t (the AdvDiff special case with V replaced by u); Bratu u'' + lambda e^u = 0 is k = 1, ae = lambda; Allen-Cahn
 * eps^2 lap u + u - u^3 = f is k = eps^2, s = 1, a3 = -1.
 * Out of scope: the strong form (a solution-dependent diffusion coefficient: hpv_set_quasilinear; trainable coefficients: hpv_set_trainable; hpv_set_collocation*,
 * hpv_residual_points, hpv_element_indicators stay refused as for the linear class).  exp(u) is not guarded against overflow.
 *
 * coef is [M][n_owned*qx*qy] in planes, M = 4 in 1-D in the order (a2, a3, ae, g), M = 5 in 2-D in the order (a2, a3, ae, gx, gy),
 * the layout of hpv_set_operator; n = M*n_owned*qx*qy.  A plane that is zero at every owned point switches its term off: it is
 * not evaluated at all (gx and gy count as one term).  NULL with n = 0, or planes that are all zero, remove the term: the handle
 * then runs k_project_lin again and computes bit for bit what a handle that never had the term computes.
 * Everything is copied.  Waits for the handle's stream and drops the captured iteration graphs (like hpv_set_operator).
 * hpv_set_elements / hpv_set_element_boxes invalidate the planes: a handle that HAD a term then answers -3 from a pass
 * ("hpv_set_nonlinear has not been called again") until the planes are set again or removed -- it never silently trains the
 * linear problem.  The planes are not state: hpv_get_state / hpv_set_state do not carry them.
 * hpv_kernel_variant names the kernel and the active terms, e.g. k_project_nl<6x5/4x3;u2,u3,exp,adv>; hpv_pass_structure stays 0.
 * Returns 0; -1 for a handle of another problem, a wrong n, a non-finite value, a shape beyond the kernel's LDS; -3 before
 * hpv_set_elements; -2 on a HIP error. */
int hpv_set_nonlinear(hpv_handle h, const double* coef, size_t n);

/* Quasilinear diffusion on a handle of the class above: the diffusive flux is scaled by a multiplier that depends on the solution,
 *
 *     div( mu(x; u, s) K grad u ) + b . grad u + s u + N(x; u, grad u) = f
 *     s = |grad u|^2 = u_x^2 [+ u_y^2]       mu = P(u) B(s)       P = m0 + m1 u + m2 u^2       B = (delta + s)^r
 *
 * with K the scalar, diagonal or full tensor of hpv_set_operator / hpv_set_operator_tensor, m0, m1, m2, delta given per quadrature
 * point and r one scalar per handle.  k(u) = 1 + u^2 is m = (1, 0, 1), r = 0; the regularised p-Laplacian m = (1, 0, 0),
 * delta = eps^2, r = (p - 2) / 2; the minimal-surface equation delta = 1, r = -1/2.  On unit elements (hpv_set_element_points) u_x,
 * u_y are the physical derivatives and the geometry sits in the folded tensor, so s is the physical |grad u|^2 and the planes are
 * handed as they are, NOT times det A.  mu multiplies the two flux integrands of R; the gradient follows by the chain rule at the
 * point (the _q instantiations of k_project_nl, csrc/kernels_nonlin.hip; the same LDS, no further launch).
 *
 * planes is [4][n_owned*qx*qy] in the order (m0, m1, m2, delta), the layout of hpv_set_operator; n = 4*n_owned*qx*qy.  The factor P is
 * evaluated unless m0 == 1 and m1 == m2 == 0 at every owned point, the factor B iff exponent != 0 (then delta > 0 is required at
 * every point, zero-weight padding points included; otherwise delta is not read).  NULL with n = 0, or planes and an exponent that
 * leave both factors 1, remove the term: nothing is kept and the handle launches bit for bit what it launched before the call.
 * No check is made that P(u) stays positive.
 * Everything is copied.  Waits for the handle's stream and drops the captured iteration graphs, like hpv_set_nonlinear.
 * hpv_set_elements / hpv_set_element_boxes / hpv_set_element_points invalidate the planes: a handle that HAD the term then answers -3
 * from a pass ("hpv_set_quasilinear has not been called again") until the planes are set again or removed.  The planes are not state.
 * hpv_kernel_variant carries ";quasi", e.g. k_project_nl<6x5/4x3;u3;quasi;tensor>.  The divergence-form strong residual
 * (hpv_set_strong_form_div, hpv_linear_indicators) carries the multiplier; the elementwise one (hpv_set_strong_form) refuses with -3
 * while the term is set, and hpv_residual_norm's energy metric is the caller's choice of Gram factors as before.
 * Returns 0; -1 for a wrong n, a non-finite plane entry (named) or exponent, exponent != 0 with a delta <= 0 (named), a shape beyond the
 * kernel's LDS; -3 for a handle of another problem, a handle with trainable coefficients (hpv_create_ex with n_coef > 0; and
 * hpv_set_trainable refuses with -3 on a handle with the term), or before hpv_set_elements; -2 on a HIP error. */
int hpv_set_quasilinear(hpv_handle h, const double* planes, size_t n, double exponent);

/* Integral constraints on a handle of the class above: up to HPV_MAX_MOMENTS weighted moments of u over the handle's Nq = n_owned*qx*qy
 * quadrature points and a quadratic penalty on each,
 *     I_k   = sum_q m_k[q] u_q^p_k            p_k in {1, 2}
 *     pen_k = w_k (I_k - c_k)^2               lossv += sum_k pen_k
 *     d loss / d u_q += 2 w_k (I_k - c_k) p_k u_q^(p_k - 1) m_k[q]
 * u is what the projection kernel reads (with hpv_set_ansatz: G + D N).  m_k is a ready-made measure plane in the layout of
 * hpv_set_operator: density x tensor quadrature weight x |J_e| (x det A on unit elements, hpv_set_element_points); the caller builds
 * it.  A zero-weight padding point has m_k = 0: it adds 0 to I_k and receives exactly 0.  A prescribed mean or mass, the
 * normalisation int u^2 = 1 and the deflation integrals int u v_j = 0 of an eigenvalue problem are all this term.
 * Three launches follow the projection kernel (k_moment_part, k_moment_close, k_moment_adj; csrc/kernels_moment.hip; the first two in
 * hpv_eval_loss), inside the captured iteration graphs; no atomics, the same bits from call to call.  The penalties are part of the
 * first entry of the loss triple.  hpv_kernel_variant carries ";mom=K" in the projection kernel's bracket.
 *
 * power, target, weight are [n_terms]; measure is [n_terms][Nq], n = n_terms*Nq.  n_terms == 0 (the arrays may be NULL) removes the
 * terms: nothing is kept, and the handle launches bit for bit what a handle that never had terms launches.
 * Everything is copied.  Waits for the handle's stream and drops the captured iteration graphs, like hpv_set_nonlinear.
 * hpv_set_elements / hpv_set_element_boxes / hpv_set_element_points invalidate the planes: a handle that HAD terms then answers -3
 * from a pass ("hpv_set_moments has not been called again") until they are set again or removed.  The terms are not state.
 * Returns 0; -1 for n_terms outside 0..HPV_MAX_MOMENTS, a power outside {1, 2}, a negative weight, a wrong n, a non-finite target,
 * weight or measure entry; -3 for a handle of another problem (a linear handle exists under the variational scheme only: hpv_create), before hpv_set_elements, and with n_terms > 0 on a handle with
 * an exchange connected (hpv_rccl_connect, hpv_p2p_export / _connect -- which in turn refuse with -3 while terms are set: I_k is a
 * global integral and there is no collective before the adjoint; n_terms == 0 is accepted there, and where no terms are set it touches
 * nothing); -2 on a HIP error. */
#define HPV_MAX_MOMENTS 8
int hpv_set_moments(hpv_handle h, int n_terms, const int* power, const double* measure, size_t n, const double* target, const double* weight);
/* I_k and pen_k of the most recent pass (waits for the handle's stream); n_terms must equal the handle's count.  Returns 0; -1 otherwise. */
int hpv_read_moments(hpv_handle h, double* values, double* penalties, int n_terms);

/* Coefficient identification on a handle of the class above: n_coef trainable scalars c_0 .. c_{n_coef-1} follow the network
 * parameters in theta (1 <= n_coef <= HPV_MAX_COEF) and are trained with them.  Each scalar owns a DIRECTION D_m in the space of
 * all coefficient planes; the planes the projection uses are
 *     plane_p(x_q) = base_p(x_q) + sum_m c_m D_m,p(x_q)
 * with p over the operator planes (k, b, s | kx, ky, bx, by, s) followed by the nonlinear planes (a2, a3, ae, g | a2, a3, ae, gx,
 * gy) and base what hpv_set_operator / hpv_set_nonlinear hold.  Isotropic conductivity: D = 1 in kx and ky; piecewise-constant
 * conductivity: indicator functions of subdomains; Burgers viscosity: D = -1 in kx; Bratu lambda: D = 1 in ae; wavenumber squared:
 * D = 1 in s.  The coefficients enter the variational term only (the data and flux terms add nothing to their gradient), and
 *     d lossv / d c_m = sum_e sum_q [ (D_s u + D_bx u_x + D_by u_y + D_a2 u^2 + D_a3 u^3 + D_ae e^u + u (D_gx u_x + D_gy u_y)) Gbar_0
 *                                     + D_kx u_x Gbar_1 + D_ky u_y Gbar_2 ]
 * with Gbar_t the adjoints of the three integrands (k_project_id, csrc/kernels_ident.hip).
 * Out of scope: positivity constraints or reparametrised coefficients, coefficients given by a second network, the strong form,
 * coefficients in the data or flux term.
 *
 * hpv_create_ex is hpv_create with n_coef such slots (hpv_create is this call with 0; such a handle computes bit for bit what it
 * always did).  Ptot = P + (epsilon of AdvDiff) + n_coef: hpv_num_params, hpv_set_params / hpv_get_params, hpv_get_state /
 * hpv_set_state, the gradient of hpv_loss_and_grad and hpv_reduce_buffer carry the slots behind the network.  The history's fourth
 * column (eps_hist of hpv_step_record / hpv_history_read) reports theta[P], the FIRST coefficient.  n_coef > 0 is refused (-1) for
 * any other pde and above HPV_MAX_COEF.
 *
 * hpv_set_trainable: dirs is [n_coef][K + M][n_owned*qx*qy] in the plane order above and the layout of hpv_set_operator; n is the
 * exact count.  Everything is copied.  A (m, p) plane that is zero at every owned point is never read on the device; a direction
 * that touches a nonlinear plane makes that term active even where its base plane is zero or was never given.  Waits for the
 * handle's stream and drops the captured iteration graphs.  hpv_set_elements / hpv_set_element_boxes invalidate the directions:
 * a pass on a handle created with n_coef > 0 answers -3 until they are set (again) -- it never silently trains fixed coefficients.
 * The directions are not state.  hpv_kernel_variant names the kernel, the active terms and the count, e.g.
 * k_project_id<6x5/4x3;u3;nc=2>; hpv_pass_structure stays 0.
 * Returns 0; -1 for a handle without such slots, a wrong n, NULL, a non-finite value; -3 before hpv_set_elements; -2 on a HIP error. */
#define HPV_MAX_COEF 8
int hpv_create_ex(hpv_handle* out, const hpv_config* cfg, int n_coef);
int hpv_set_trainable(hpv_handle h, const double* dirs, size_t n);

/* A full diffusion tensor on a 2-D handle of the class above (HPV_PDE_LINEAR2D only):
 *     L u = div(K grad u) + bx u_x + by u_y + s u = f          K = [[kxx, kxy], [kyx, kyy]] per quadrature point, not necessarily symmetric
 * so that media whose principal axes are not the coordinate axes (rotated anisotropy, layers, fibres) can be stated.  Of the three
 * integrands of hpv_set_operator only two change,
 *     G1 = kxx u_x + kxy u_y          G2 = kyx u_x + kyy u_y
 * tables, the constants of the element, masking, F, lossv and the loss triple are unchanged; the TENSOR instantiations of
 * k_project_lin / k_project_nl / k_project_id run (the same LDS, no atomics, the same bits from call to call) and hpv_kernel_variant
 * carries ";tensor" inside the brackets, e.g. k_project_lin<6x5/4x3;tensor> or k_project_id<6x5/4x3;u3;tensor;nc=2>.
 *
 * coef is [7][n_owned*qx*qy] in the order (kxx, kxy, kyx, kyy, bx, by, s), each plane laid out as in hpv_set_operator, whose contract
 * this call follows: everything is copied, it waits for the handle's stream and drops the captured iteration graphs, new elements
 * invalidate the planes.  The operator call made LAST decides which kernels run: a later hpv_set_operator returns the handle to the
 * diagonal kernels and their exact variant names.  On a tensor handle hpv_set_trainable takes [n_coef][7 + 5][n_owned*qx*qy] (the
 * seven planes above, then the nonlinear ones) and d lossv / d c_m gains D_kxy u_y Gbar_1 + D_kyx u_x Gbar_2; otherwise [5 + 5].
 * Switching between the two operator calls invalidates the directions: a pass answers -3 until they are set again.
 * Out of scope while the operator is a tensor: the ELEMENTWISE strong form -- it would need u_xy -- so hpv_set_strong_form is refused
 * (-1, the handle stays usable), and hpv_linear_indicators unless the divergence form is set (hpv_set_strong_form_div, which needs
 * no u_xy); 1-D handles; a solution-dependent tensor.
 * Returns 0; -1 for a handle of another problem, a wrong n, NULL, a non-finite value; -3 before hpv_set_elements; -2 on a HIP error. */
int hpv_set_operator_tensor(hpv_handle h, const double* coef, size_t n);

/* Mapped (non-box) elements on a 2-D handle of the class above: the elements are UNIT elements -- J = Jx = Jy = 1 -- whose
 * quadrature points are the caller's.  X is [n_total][2][qy*qx] (per element the x plane, then the y plane, q = j*qx + i): the
 * PHYSICAL images of the reference nodes under each element's map.  The geometry is the caller's to fold into the planes: with
 * A = d(x,y)/d(xi,eta) at a point, d = det A > 0 and M = adj(A), the weak form on the element pulled back to the reference square is
 * that of a unit element with K_eff = M K (a full tensor: hpv_set_operator_tensor), b_eff = d b, s_eff = d s, a_eff = d a for every
 * nonlinear plane, D_eff likewise for every direction and f_eff = d f; u, u_x, u_y stay the network's physical derivatives at the
 * physical points, so the data term, the flux term and hpv_set_ansatz need nothing.  hpv_assemble_rhs on such a handle returns
 * sum_q w_q f_q phi_r phi_k.  Quadrilaterals with straight or curved sides, polar or any other smooth coordinates are all this call.
 * Slicing by [e_begin, e_end), preconditions, the re-slicing of F and of the counts, and the invalidation of every plane are those
 * of hpv_set_element_boxes (both end in one function); hpv_set_elements / hpv_set_element_boxes return the handle to boxes.
 * The points are checked to be finite; the maps themselves never reach the library and are not checked.
 * Out of scope on such a handle: the TABLE dual norm -- the Gram matrix of the reference square is not the physical H^1 inner product --
 * so hpv_set_residual_norm(dual) is refused on it and this call is refused while that norm is set (the dense factors of
 * hpv_set_residual_gram carry the physical product: under them this call is accepted and drops the factors); the ELEMENTWISE strong
 * form: hpv_set_strong_form is refused on it and this call is refused while that form is set (the divergence form,
 * hpv_set_strong_form_div, works on such a handle: this call then orphans its 1 / det A); 1-D handles; triangles.
 * Returns 0; -1 for another kind of handle, NULL, n_total < 1, a bad range, a non-finite point, the two refusals above; -3 before
 * hpv_set_quadrature / hpv_set_tables; -2 on a HIP error. */
int hpv_set_element_points(hpv_handle h, const double* X, int n_total, int e_begin, int e_end);

/* Boundary / data points of lossb (P1:98, P2:122, P3:184): X is [n][dim] row-major, u is [n].
 * The term is weighted by cfg.lossb_weight.  n = 0 disables it (ranks other than 0). */
int hpv_set_data(hpv_handle h, const double* X, const double* u, int n);

/* Flux term: Neumann / Robin conditions and derivative observations as a penalty at points (an extension; the test functions
 * vanish on every element boundary, so the weak forms carry no natural boundary condition).  With
 *   r_p = a_p u(X_p) + b_p . grad u(X_p) - g_p,   grad = (u_x) in 1-D, (u_x, u_y) in 2-D, (u_x, u_t) for AdvDiff,
 *   lossf = weight * mean_p(r_p^2),   loss = lossb_weight * lossb + lossf + lossv   (lossp for lossv under scheme PINNs).
 * Neumann: a = 0, b = the outward normal; Robin: both non-zero; a derivative sensor: b = e_c; a = 1, b = 0 is the value term.
 * X is [n][dim], coef is [n][1 + dim] = (a, b_0 .. b_{dim-1}), both row-major; g is [n].  Everything is copied.  n = 0 removes the
 * term (ranks other than 0 of a multi-GPU run: the term lives on rank 0 like the data term); the handle then computes bit for bit
 * what a handle that never had the term computes.  Epsilon of AdvDiff does not enter: its gradient slot gets nothing from the term.
 * Side effects: waits for the handle's stream, drops the captured iteration graphs (like hpv_set_data), re-creates the term's
 * point batch.  The data sets are not state: hpv_get_state / hpv_set_state do not carry them.
 * Where the sums go: the packed buffer's slot [Ptot + 1] and the history's second column hold lossb_weight * msq + weight * msf
 * (so `loss` = loss3[0] includes the term and the multi-GPU reduce layout keeps its size); slot [Ptot + 2] stays the plain msq.
 * loss3[1] therefore is lossb_weight * lossb + lossf for AdvDiff (which reports the weighted slot, P3:184) and stays the plain
 * mean of the Dirichlet term for the Poisson problems (P1:98, P2:122); hpv_read_flux_loss returns the term on its own.
 * Returns 0; -1 for a NULL handle, negative n, a NULL array with n > 0, a non-finite weight; -2 on a HIP error. */
int hpv_set_flux_data(hpv_handle h, const double* X, const double* coef, const double* g, int n, double weight);
/* sync + copy: out2 = {weight * msf, msf}, msf = mean_p(r_p^2) of the most recent pass (forward-only or reverse-mode) on this
 * handle; {0, 0} without the term or before the first pass.  Returns 0; -1 for NULL arguments; -2 on a HIP error. */
int hpv_read_flux_loss(hpv_handle h, double* out2);

/* Collocation points of the strong-form PINN branch (`scheme == 'PINNs'`, P2:124-129): lossp = mean(r^2)
 * over the points X [n][dim] replaces the variational term, loss = lossb_weight * lossb + lossp (P2:129).  Residual per problem:
 *   Poisson-1D  r = -u_xx - f                        (net_f, P1:150-155, against f_train as P2:124)
 *   Poisson-2D  r = u_xx + u_yy - f                  (P2:187-194)
 *   AdvDiff     r = u_t + V u_x - epsilon u_xx - f   (net_f, P3:247-253, lossp P3:186; columns of X are (x, t), V = cfg.V)
 * The reference offers the switch in P2 only; the other two follow P2:124-129.  f is [n]; NULL means a zero right-hand side and
 * is accepted for AdvDiff only (as hpv_set_rhs does for its variational form).  AdvDiff: epsilon stays the trainable last
 * parameter, read on the device at every pass; d lossp / d epsilon = (2 / n_total) sum r (-u_xx) lands in the packed buffer's
 * d-epsilon slot like the variational path's. */
int hpv_set_collocation(hpv_handle h, const double* X, const double* f, int n);
/* One rank's shard of the collocation set (multi-GPU PINN branch): n points here, n_total over all ranks -- lossp is the
 * mean over all n_total points (P2:124), the partial sums are made global by the iteration's all-reduce. */
int hpv_set_collocation_shard(hpv_handle h, const double* X, const double* f, int n, long n_total);

size_t hpv_num_params(hpv_handle h);
int hpv_set_params(hpv_handle h, const double* theta, size_t n); /* also resets Adam state (P1:107) */
int hpv_get_params(hpv_handle h, double* theta, size_t n);

/* loss3 = {loss, lossb (as the reference reports it), lossv} at the current parameters, and
 * d loss / d theta (grad may be NULL).  Replaces the forward/backward graph of P1:64-104. */
int hpv_loss_and_grad(hpv_handle h, double* loss3, double* grad_or_null);

/* n_iters Adam iterations = n_iters x `sess.run(train_op_Adam)` (P1:208, P2:242, P3:309), all
 * device-resident; loss3_after (may be NULL) is the loss evaluated AFTER the last update, which
 * is what the reference records (P1:211, P2:243, P3:315). */
int hpv_step(hpv_handle h, int n_iters, double* loss3_after);

/* n_iters Adam iterations with the loss after EVERY update recorded -- what VPINN.train of the 2-D script does with a
 * second forward pass per iteration (P2:243-244).  The loss after update k is the value the forward pass of
 * iteration k+1 computes anyway; every training iteration appends it to a device-side history, so only the loss after
 * the last update costs a forward pass.  loss3_hist is [n_iters][3] = {loss, lossb, lossv} after update 1..n_iters;
 * eps_hist (may be NULL) is [n_iters], the trainable diffusion coefficient after each update (P3:318, 0 for the Poisson
 * problems; theta[P], the first coefficient, on a handle of hpv_create_ex).  hpv_history_reset / hpv_history_read expose the history to callers that drive the iterations themselves
 * (multi-GPU: entry i = loss / epsilon seen by the i-th forward pass since the reset, global after the all-reduce). */
int hpv_step_record(hpv_handle h, int n_iters, double* loss3_hist, double* eps_hist);
int hpv_history_reset(hpv_handle h);
int hpv_history_read(hpv_handle h, int n, double* loss3_hist, double* eps_hist);

/* Pieces of hpv_step for the multi-GPU path (one process per GPU): enqueue forward + backward
 * into the packed device buffer [grad (P) | lossv | lossb | pad] (all partial sums of this
 * shard), let the caller all-reduce that buffer over RCCL, then apply the TF1 Adam update.
 * hpv_reduce_buffer returns the device pointer and length (in doubles) of that buffer. */
int hpv_forward_backward(hpv_handle h);
int hpv_reduce_buffer(hpv_handle h, void** dev_ptr, size_t* n_doubles);
int hpv_apply_adam(hpv_handle h);
/* Multi-GPU default: the all-reduce issued by the library itself.  One process per GPU; the handle owns an RCCL
 * communicator and every training iteration of hpv_step / hpv_step_record is forward+backward -> ONE
 * ncclAllReduce(sum) of the packed buffer [grad (P) | d eps | lossv | w*lossb | msq | pad] over xGMI -> TF1 Adam, all
 * enqueued on the handle's stream and captured into its iteration graphs.  After hpv_rccl_connect,
 * hpv_step / hpv_step_record / hpv_loss_and_grad are collective calls: every rank issues the same sequence.
 *   hpv_rccl_available: local check that every rank runs (and agrees on) BEFORE anyone enters the collective calls below;
 *   hpv_rccl_unique_id: rank 0 creates the 128-byte ncclUniqueId; the caller distributes it to all ranks;
 *   hpv_rccl_connect  : ncclCommInitRank (collective);
 *   hpv_rccl_selftest : known-answer all-reduce (collective); out[i] must equal W(W+1)/2 + W*1e-3*i;
 *   hpv_exchange_in_use: 0 none (single GPU or caller-driven pieces above), 1 RCCL, 2 peer-mapped mailboxes (below). */
int hpv_rccl_available(void);   /* 1 when librccl and its entry points can be loaded in this process (local, not collective) */
int hpv_rccl_unique_id(hpv_handle h, void* id128);
int hpv_rccl_connect(hpv_handle h, int world, int rank, const void* id128);
int hpv_rccl_selftest(hpv_handle h, double* out, size_t n);
int hpv_rccl_disconnect(hpv_handle h);
/* The caller stopped waiting for a hpv_rccl_connect / hpv_rccl_selftest that blocks on a helper thread (wall-clock bound of the
 * communicator set-up).  The ONLY entry point that may be called while another thread is inside the library on the same
 * handle: the abandoned call returns -6 and never touches the handle again (a communicator that comes up late is destroyed).
 * After an abandoned connect the handle stays usable, unconnected; after an abandoned self-test its stream may sit behind a
 * collective that never completes -- do not use that handle again (and do not destroy it while the call is still inside). */
int hpv_rccl_abandon(hpv_handle h);
int hpv_exchange_in_use(hpv_handle h);
/* Evidence for a reader of the benchmark line (the ONE collective of the path, lossv = sum_e loss_e of P2:120):
 *   hpv_rccl_info          : world size and rank as the COMMUNICATOR reports them (ncclCommCount / ncclCommUserRank);
 *                            0 / -1 when no communicator is connected.  Local call.
 *   hpv_rccl_time_allreduce: the all-reduce of the packed buffer ALONE -- `reps` eager calls on a scratch buffer of the same
 *                            size, one hipEvent pair around them, microseconds per call on this rank.  Collective. */
int hpv_rccl_info(hpv_handle h, int* world, int* rank);
int hpv_rccl_time_allreduce(hpv_handle h, int reps, double* avg_us);
/* Opt-in alternative (HPV_EXCHANGE=p2p in the Python classes): in-library exchange over peer-mapped mailboxes instead of
 * a collective-library call every iteration: each rank owns a mailbox that every peer maps through hipIpc; one kernel per
 * iteration writes the buffer into all mailboxes over xGMI, waits for the peers' contributions (bounded), sums them in
 * rank order -- bitwise identical on all ranks -- and applies the Adam update.  After hpv_p2p_connect, hpv_step /
 * hpv_step_record / hpv_loss_and_grad are collective calls: every rank must issue the same sequence.
 *   hpv_p2p_export  : allocate the mailbox, return its two 64-byte IPC handles (handles128);
 *   hpv_p2p_connect : handles = [world][128], the exports of all ranks in rank order (all-gathered by the caller);
 *   hpv_p2p_selftest: known-answer exchange (collective); out[i] must equal W(W+1)/2 + W*1e-3*i, *timed_out 0. */
int hpv_p2p_export(hpv_handle h, int world, int rank, void* handles128);
int hpv_p2p_connect(hpv_handle h, const void* handles);
int hpv_p2p_selftest(hpv_handle h, double* out, size_t n, int* timed_out);
int hpv_p2p_disconnect(hpv_handle h);
int hpv_eval_loss(hpv_handle h);            /* forward only -> same packed buffer slots [P], [P+1] */
int hpv_read_loss(hpv_handle h, double* loss3); /* sync + copy {loss, lossb, lossv} from the buffer   */
int hpv_sync(hpv_handle h);

/* u at arbitrary points: VPINN.predict (P1:197-199, P2:255-257).  X is [n][dim] row-major. */
int hpv_predict(hpv_handle h, const double* X, int n, double* u_out);

/* Device-side validation.  What the reference does with a trained network goes through the host and yields u only: VPINN.predict
 * on the test grid (P1:197-199, P2:255-257), the norm taken in numpy; its pointwise PDE residual is net_f (P2:187-194, P3:247-253).
 * The entry points below keep that on the device: derivative channels and the strong residual at the caller's own points, the error
 * norms against an exact solution on a stored validation set, and a device-side history of those norms that is filled BETWEEN training
 * iterations without a host round trip -- the error-versus-iteration curve of a convergence study at the cost of one forward launch
 * and one reduction launch per sample.  Both schemes, both backends, every network shape the handle accepts.
 *
 * hpv_eval_points: the FULL channel list at n arbitrary points, out = [C][n]: u, u_x, u_xx (C = 3) in 1-D; u, u_x, u_y (u_t), u_xx,
 *   u_yy (u_tt) (C = 5) in 2-D and for AdvDiff -- net_u / net_du / net_dxu / net_dyu / net_dtu of the classes (P1:140-148, P2:171-185,
 *   P3:232-245).  One forward launch on a batch the handle owns (re-created only when n changes).  n_out = C * n.
 * hpv_residual_points: the strong residual at n arbitrary points, in either scheme, with the formulas of hpv_set_collocation
 *   (-u_xx - f | u_xx + u_yy - f | u_t + V u_x - epsilon u_xx - f); epsilon is read from the device parameters; f NULL = zero. */
int hpv_eval_points(hpv_handle h, const double* X, int n, double* out, size_t n_out);
int hpv_residual_points(hpv_handle h, const double* X, const double* f_or_null, int n, double* r_out);
/* The validation set, uploaded once: points X [n][dim], exact values u [n] and, optionally, exact gradients du [n][dim]; n = 0
 * clears it.  In a multi-GPU run every rank holds the whole set and evaluates it redundantly (the parameters are identical on all
 * ranks: no collective).
 * hpv_validate: one forward launch over the set (value only; value and first derivatives when du was given) and ONE reduction
 *   launch; out6 = {sum (u^ - u)^2, sum u^2, max |u^ - u|, sum |grad u^ - grad u|^2, sum |grad u|^2, n}, the two gradient sums 0
 *   without du.  fp64 throughout, a summation order that depends on n alone: the six numbers are bitwise reproducible from run to run
 *   and from rank to rank.  -3 without parameters or without a validation set. */
int hpv_set_validation(hpv_handle h, const double* X, const double* u, const double* du_or_null, int n);
int hpv_validate(hpv_handle h, double* out6);
/* Device-side history of those six numbers, modelled on hpv_history_*: hpv_validate_enqueue launches the forward and the reduction on
 * the handle's stream and appends at a device-side index -- no synchronisation, no host read (callers that drive the iterations
 * themselves put it between them); hpv_validation_read copies the first n entries since the reset, out = [n][6] (the history holds
 * 4096 entries, later ones are dropped; -3 when fewer than n were enqueued). */
int hpv_validation_reset(hpv_handle h);
int hpv_validate_enqueue(hpv_handle h);
int hpv_validation_read(hpv_handle h, int n, double* out);
/* n_iters Adam iterations as hpv_step runs them, with a validation enqueued after every `every`-th update and nothing read back
 * until the end: out = [n_iters / every][6] (n_out doubles available); a remainder n_iters % every is trained, not validated.  The
 * iterations run in chunks of `every` (graph replays where hpv_step replays them; the validation launches sit between the replays),
 * so the parameters are bit for bit those of `hpv_step(every)` repeated.  Collective after hpv_rccl_connect / hpv_p2p_connect like
 * hpv_step, and with its handling of an exchange timeout.  -1: every < 1, n_out too small, more samples than the history holds. */
int hpv_step_validate(hpv_handle h, int n_iters, int every, double* out, size_t n_out);

/* L-BFGS stage after Adam (an extension; no reference counterpart): up to max_iter quasi-Newton iterations on ALL num_params
 * entries of theta -- the network, AdvDiff's epsilon, the trainable coefficients of a handle made with n_coef > 0 -- on every
 * problem class and both schemes.  The optimiser's vectors (the iterate, the gradient, the direction, the rings of up to `history`
 * pairs s, y) stay on the device; the line search runs on the host over scalars.  One function evaluation is one backward pass of
 * the handle plus a read-back of 32 bytes; launches are eager (the captured iteration graphs of the Adam path are neither used nor
 * dropped).  The algorithm and its decisions are those of torch.optim.LBFGS with line_search_fn = "strong_wolfe": two-loop
 * recursion scaled by (y.s)/(y.y) of the newest pair, a pair kept only when y.s > 1e-10, strong-Wolfe search with c1 = 1e-4,
 * c2 = 0.9 and at most 25 steps (and never more than the evaluations max_eval leaves), first step min(1, 1/|g|_1) lr and lr
 * afterwards, exits on max|g| <= tolerance_grad, g.d > -tolerance_change, max|t d| <= tolerance_change and
 * |f - f_prev| < tolerance_change.
 *   opts: history 1 .. 64 (larger values are capped; torch's 100 is too large for here, the bindings default to 20); max_eval <= 0
 *     means max_iter * 5 / 4; torch's defaults otherwise: lr 1, tolerance_grad 1e-7, tolerance_change 1e-9.
 *   loss3_hist (may be NULL): [max_iter + 1][3] = {loss, lossb, lossv} at the starting point and after every accepted iteration
 *     (iters + 1 rows are written); by the sufficient-decrease condition the first column never increases.
 *   info (may be NULL): {iterations taken, function evaluations, pairs skipped by the curvature test, HPV_LBFGS_* reason}.
 * A search that ends without an acceptable point -- 25 steps or the evaluation budget used up, a non-finite loss -- is not an
 * error: the parameters are set back to the last accepted iterate bit for bit, the reason says which, the call returns 0.
 * Adam's state is left alone: the moments m and v, the beta powers and the update count are what they were, and a later training
 * call continues Adam from ITS state at the new parameters.  The history of pairs survives between calls (a second call goes on
 * where the first stopped) and changes of the mesh, rule or data (theta keeps its meaning); it is dropped by the reset call below
 * and whenever parameters are handed in (set_params, set_state), and it is not part of the checkpoint.
 * -4 with a message: a handle with an exchange connected (hpv_exchange_in_use != 0) or holding a shard of the model (part of the
 * elements or of the collocation points) -- one GPU only; history < 1.  Pass errors come back as they are. */
typedef struct hpv_lbfgs_opts {
    int history, max_iter, max_eval;
    double lr, tolerance_grad, tolerance_change;
} hpv_lbfgs_opts;
enum { HPV_LBFGS_MAX_ITER = 0,        /* max_iter iterations were taken                                             */
       HPV_LBFGS_MAX_EVAL = 1,        /* the evaluation budget ran out (inside a search: parameters set back)      */
       HPV_LBFGS_TOL_GRAD = 2,        /* max|g| <= tolerance_grad                                                   */
       HPV_LBFGS_TOL_CHANGE = 3,      /* step or decrease below tolerance_change, or the bracket closed on t = 0   */
       HPV_LBFGS_TOL_DIRECTION = 4,   /* g.d > -tolerance_change: no descent left along the direction              */
       HPV_LBFGS_MAX_LS = 5,          /* 25 search steps without a Wolfe point (parameters set back)               */
       HPV_LBFGS_NONFINITE = 6 };     /* the loss is not finite (parameters set back)                              */
int hpv_lbfgs_step(hpv_handle h, const hpv_lbfgs_opts* opts, double* loss3_hist, int* info);
int hpv_lbfgs_reset(hpv_handle h);   /* drop the history of pairs; the next iteration steps along -g */

/* Checkpoint / resume (the reference never saves weights): the packed state
 * [theta | Adam m | Adam v | beta1^t | beta2^t], 3*num_params+2 doubles; a resumed run continues bit-exactly. */
int hpv_get_state(hpv_handle h, double* buf, size_t n);
int hpv_set_state(hpv_handle h, const double* buf, size_t n);

/* Driver-side RHS assembly on the device: F_ext[e][k][r] = J_e sum_q w phi_r phi_k f(x_q)
 * (P1:277-291, P2:386-411) for the owned elements from f at the handle's quadrature points
 * (element-major, q = j*qx+i, n = n_owned*qx*qy); F_out is [n_owned][nty][ntx]. */
int hpv_assemble_rhs(hpv_handle h, const double* f_quad, size_t n, double* F_out, size_t n_out);

/* Driver-side table generation on the device.  hpv_gll_rule: the Q-point Gauss-Lobatto-
 * Legendre nodes and weights the drivers take from GaussLobattoJacobiWeights(Q, 0, 0) (Q:47-61; P1:312, P2:355,
 * P3:395), Newton on the three-term recurrence.  hpv_test_tables: phi_n = P_{n+1} - P_{n-1}, phi'_n, phi''_n for
 * n = 1..ntest at the nodes xi (VPINN.Test_fcn / dTest_fcn, P1:157-183) as [3][ntest][q], the layout
 * hpv_set_tables takes per direction. */
int hpv_gll_rule(hpv_handle h, int q, double* xi, double* w);
int hpv_test_tables(hpv_handle h, int ntest, const double* xi, int q, double* tab);

/* Introspection for tests / benchmarks. */
int hpv_get_residuals(hpv_handle h, double* R, size_t n);   /* R of the owned elements [ne][nty][ntx] */

/* Per-element refinement indicators of the owned elements at the CURRENT parameters; variational scheme only.
 * out = [n_owned][HPV_IND_N]:
 *  0 loss_e  = mean over the element's ACTIVE test functions of R^2  (the term the training pass sums into lossv)
 *  1 eta2_e  = J_e * sum_q w_q r_q^2, r the strong residual of hpv_set_collocation
 *              (-u_xx - f | u_xx + u_yy - f | u_t + V u_x - eps u_xx - f), eps read from the device parameters
 *  2 sumR2_e = sum of R^2 over the active block
 *  3 topx_e  = sum of R^2 over the highest active x index (r == nax_e - 1)
 *  4 topy_e  = the same for the highest active y / t index (k == nay_e - 1); 0 in 1-D
 * f_quad: f at the handle's own quadrature points, element-major, q = j*qx + i, n = n_owned*qx*qy (the layout of
 * hpv_assemble_rhs); NULL = zero right-hand side (n is then ignored).
 * Launches, all on the handle's stream with one synchronisation at the end: the forward-only pass of hpv_eval_loss (which makes R
 * current), one forward-only launch of the full channel list on the quadrature batch's own points, one k_elem_indicators launch
 * (one workgroup per element; fixed summation order, no atomics: the result is bitwise reproducible from call to call), one copy.
 * The first step needs no special structure: a forward-only pass never runs a whole-iteration kernel (SPLIT mode and k_iter_tall
 * exist for reverse-mode passes only), it is always forward + projection, and every projection kernel stores R of all owned
 * elements.  Like hpv_eval_loss it overwrites the loss slots of the packed buffer.  Zero-weight padding points of a padded rule
 * contribute exactly 0.  Refused (negative status, hpv_last_error; the handle stays usable): the strong-form scheme, a handle
 * without parameters / elements, wrong n or n_out. */
#define HPV_IND_N 5
int hpv_element_indicators(hpv_handle h, const double* f_quad_or_null, size_t n, double* out, size_t n_out);

/* Refinement indicators for the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D, with or without hpv_set_nonlinear / hpv_set_trainable).
 * ADDS an opt-in beside hpv_element_indicators, which stays refused on these handles as do hpv_residual_points and
 * hpv_set_collocation*; it replaces nothing, and a handle that never calls hpv_set_strong_form behaves as it always did.
 * The strong residual of the class takes derivatives of the diffusion planes,
 *     r = kx u_xx + (d kx/dx) u_x + ky u_yy + (d ky/dy) u_y + bx u_x + by u_y + s u + N(u, grad u) - f
 *     (1-D: r = k u_xx + k' u_x + b u_x + s u + N - f;  N as in hpv_set_nonlinear, only the terms that are switched on),
 * and the planes are nodal values on each element's tensor rule: the derivative of their interpolant at the element's own points is
 *     d kx/dx [j][i] = (sum_m Dx[i][m] kx[j][m]) / Jx_e        d ky/dy [j][i] = (sum_m Dy[j][m] ky[m][i]) / Jy_e
 * with Dx, Dy the differentiation matrices of the rule's nodes on the reference interval and Jx_e, Jy_e the element's half widths.
 * ASSUMPTION: kappa is smooth inside each element.  Exact for a plane that is a polynomial of degree < q per direction on the
 * element, spectrally accurate for a smooth one, correct inside every element for a piecewise-constant one whose jumps lie on
 * element edges.  With trainable coefficients the planes are base + sum_m c_m D_m at the parameters on the device.
 *
 * hpv_set_strong_form: Dx is the qx x qx matrix (row-major) of the device rule's x nodes, Dy the qy x qy one; 1-D handles pass
 * Dy = NULL, ny = 0.  (NULL, 0, NULL, 0) removes them.  Everything is copied.  The matrices belong to the rule: hpv_set_quadrature
 * drops them, hpv_set_tables / hpv_set_elements / hpv_set_element_boxes do not.  Nothing a pass reads changes: captured iteration
 * graphs stay, and a handle computes bit for bit what one that never made the call computes.
 * Returns 0; -1 (the handle stays usable, matrices given earlier stay) for a handle of another problem, sizes that are not the
 * current rule's, a non-finite entry, a rule whose k_lin_indicators workgroup would need more than 64 KiB of LDS --
 *     8 * (n_d * qy * (qx|1) + qx * (qx|1) + [2-D: qy * (qy|1)] + 16) bytes,  n_d = 1 in 1-D, 2 in 2-D;
 * -3 before hpv_set_quadrature; -2 on a HIP error.
 *
 * hpv_linear_indicators: out, f_quad and n follow hpv_element_indicators' contract -- [n_owned][HPV_IND_N], the same five columns
 * with the same meaning, column 1 with the r above.  r_out may be NULL (n_r is then ignored); otherwise it receives r at every
 * owned quadrature point, n_r = n_owned*qx*qy, element-major, q = j*qx + i.  The launches are hpv_element_indicators' own: the
 * forward-only pass of hpv_eval_loss (R becomes current), one forward-only launch of the full channel list, one k_lin_indicators
 * launch (csrc/kernels_linadapt.hip: one workgroup per element, fixed summation order, no atomics -- bitwise reproducible from call
 * to call), one copy (two with r_out), one synchronisation.  Like hpv_eval_loss it overwrites the loss slots of the packed buffer.
 * Returns 0; -1 for a handle of another problem, before hpv_set_strong_form (the message names it), wrong n / n_out / n_r; -3
 * where a pass would (planes, nonlinear term or directions orphaned by new elements, anything not yet set); -2 on a HIP error. */
int hpv_set_strong_form(hpv_handle h, const double* Dx, size_t nx, const double* Dy, size_t ny);
int hpv_linear_indicators(hpv_handle h, const double* f_quad_or_null, size_t n, double* out, size_t n_out, double* r_out_or_null, size_t n_r);

/* The strong residual of the linear problems in DIVERGENCE form: the second kind hpv_linear_indicators can run, and the one that works
 * on every linear handle -- 1-D, diagonal, full tensor (hpv_set_operator_tensor), unit elements (hpv_set_element_points), with or
 * without an ansatz (hpv_set_ansatz), a dual norm or trainable coefficients.  The projection kernels already form the flux planes
 *     G1 = kxx u_x + kxy u_y      G2 = kyx u_x + kyy u_y      (diagonal: kx u_x, ky u_y; 1-D: k u')      G0 = bx u_x + by u_y + s u
 * at every quadrature point from u, u_x, u_y alone; the divergence of their nodal interpolant on the element's tensor rule is
 *     r_ref[j][i] = (1/Jx) sum_m Dx[i][m] G1[j][m] + (1/Jy) sum_m Dy[j][m] G2[m][i] + G0[j][i] + N[j][i] - f[j][i]
 * with the planes as the handle holds them (after the caller's fold, base + sum_m c_m D_m with trainable coefficients), N as in
 * hpv_set_nonlinear (only the terms that are switched on), Jx = Jy = 1 on unit elements, and u, u_x, u_y the values after the ansatz
 * where there is one.  No second derivative of the network, of an element map, of G or of D is needed.  On unit elements the planes
 * carry adj(A) and det A, so G1, G2 are the Piola-transformed fluxes and r_ref = det A * r: the physical residual is r = m r_ref with
 * m = inv_det = 1 / det A per point (m = 1 on boxes).  Column 1 of hpv_linear_indicators is J_e sum_q w_x[i] w_y[j] m_q r_ref_q^2,
 * the quadrature of int r^2 dx over the element; columns 0, 2, 3, 4 are what the elementwise kind writes (column 0 the dual-norm
 * loss_e under hpv_set_residual_norm / _gram); r_out receives r.  Exact where every flux component is a polynomial of degree < q per
 * direction on the element, spectrally accurate for smooth fluxes.
 *
 * Dx, nx, Dy, ny: as hpv_set_strong_form.  inv_det: NULL and 0 on a handle with boxes; on unit elements 1 / det A at the owned points,
 * n_det = n_owned*qx*qy, element-major, finite and > 0.  All NULL / 0 removes the form.  Everything is copied.  The two kinds exclude
 * each other: either call is refused (-1, with the reason) while the other kind is set.  Matrices and inv_det belong to the rule AND
 * the elements: hpv_set_quadrature, hpv_set_elements, hpv_set_element_boxes and hpv_set_element_points drop them, and
 * hpv_linear_indicators answers -3 ("hand the strong form over again") until this call is made again.  While this kind is set,
 * hpv_set_element_points and hpv_set_ansatz are accepted.  Nothing a pass reads changes: captured iteration graphs stay.
 * hpv_linear_indicators then runs the forward-only pass of hpv_eval_loss and ONE k_div_indicators launch (csrc/kernels_linadapt.hip)
 * on the channels u, u_x[, u_y] that pass left in the quadrature batch -- no further forward launch --, one copy (two with r_out), one
 * synchronisation; fixed summation order, no atomics: bitwise reproducible from call to call.
 * Returns 0; -1 (the handle stays usable, what was given earlier stays) for a handle of another problem, the other kind being set,
 * sizes that are not the current rule's / elements', a non-finite entry, an inv_det entry that is not > 0, inv_det on boxes or none on
 * unit elements, a rule whose k_div_indicators workgroup would need more than 64 KiB of LDS (the formula of hpv_set_strong_form);
 * -3 before hpv_set_quadrature / the elements; -2 on a HIP error. */
int hpv_set_strong_form_div(hpv_handle h, const double* Dx, size_t nx, const double* Dy, size_t ny, const double* inv_det_or_null, size_t n_det);

/* Exact Dirichlet (and initial) conditions by ansatz, for the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D, with or without
 * hpv_set_nonlinear / hpv_set_trainable).  The trial function is
 *     u(x) = G(x) + D(x) N(x; theta)
 * with N the network, G any function that matches the data and D a function that vanishes exactly where the condition holds
 * (D = (x - a)(b - x) on an interval, D = (1 - x^2) t for space-time Burgers): the condition is met for every theta, and the penalty
 * lossb_weight * mean((u - u_data)^2) with its weight is not needed (it may still be used: hpv_set_data stays optional).  Every loss
 * term is taken on u and its first derivatives,
 *     u_x = G_x + D_x N + D N_x        (same for y),
 * and the channel adjoints go back through the transposed map,
 *     Nbar = D ubar + D_x uxbar + D_y uybar        N_xbar = D uxbar        N_ybar = D uybar;
 * second derivatives of G and D are never needed.  Two pointwise fp64 kernels (csrc/kernels_ansatz.hip) run the map on a batch's channels
 * in place: k_ansatz_fwd behind the batch's forward launch, k_ansatz_adj in front of its reverse launch -- around k_project_lin | _nl |
 * _id on the quadrature batch (d loss / d c_m is formed from the transformed channels), around k_data_loss and k_flux_loss, and
 * between the forward launch and the reduction of hpv_validate / hpv_validate_enqueue / hpv_step_validate.  They are captured into
 * the iteration graphs like the other launches; one lane per point, no atomics: results are bitwise reproducible.
 *
 * hpv_set_ansatz: planes = [2 * (1 + dim)][n] in the order (G, G_x[, G_y], D, D_x[, D_y]) at the points of set `which`, n its exact
 * point count: HPV_ANSATZ_QUAD the owned quadrature points, element-major, q = j*qx + i (the layout of hpv_set_operator; after
 * hpv_set_elements / hpv_set_element_boxes), HPV_ANSATZ_DATA the n of hpv_set_data, HPV_ANSATZ_FLUX the n of hpv_set_flux_data,
 * HPV_ANSATZ_VALID the n of hpv_set_validation, each in the order the points were given.  Everything is copied.  (NULL, 0) removes
 * the planes of that set; a handle whose planes have all been removed computes bit for bit what one that never had any computes.
 * Side effects: waits for the handle's stream and drops the captured iteration graphs, like hpv_set_operator.  A handle with any
 * planes keeps its boundary / data points in a batch of their own (they otherwise ride in the quadrature batch's forward launch,
 * which takes their loss on raw network values), and hpv_kernel_variant appends ";ansatz" to the projection's name.  The point-set
 * calls drop their own planes: hpv_set_elements / hpv_set_element_boxes those of QUAD, hpv_set_data, hpv_set_flux_data and
 * hpv_set_validation those of their set.  A handle that has planes for any set must have them for every non-empty one: a pass
 * (hpv_loss_and_grad, hpv_step, ...) or a validation otherwise returns -3 with a message naming the set -- u and N are never mixed.
 * The planes are not state: hpv_get_state / hpv_set_state do not carry them.
 * hpv_predict, hpv_eval_points and hpv_eval_channels keep returning the RAW network N and its derivatives; the caller applies the map
 * (the Python classes do so on the host).
 * Returns 0; -1 (the handle stays usable, planes given earlier stay) for a handle of another problem, an unknown `which`, n that is
 * not the set's count, a non-finite value, and a handle on which hpv_set_strong_form is active -- the strong residual of u needs
 * second derivatives of G and D, which is out of scope; hpv_set_strong_form on a handle that has an ansatz is refused likewise (the
 * divergence form, hpv_set_strong_form_div, needs none of them and goes together with an ansatz); -3
 * for HPV_ANSATZ_QUAD before the elements are set; -2 on a HIP error.
 * Out of scope: the problems other than the linear ones and the strong-form scheme (whole-iteration kernels, second derivatives), the
 * strong-form indicators, ansatz functions with trainable parts, fusing the map into the projection kernels. */
#define HPV_ANSATZ_QUAD  0
#define HPV_ANSATZ_DATA  1
#define HPV_ANSATZ_FLUX  2
#define HPV_ANSATZ_VALID 3
int hpv_set_ansatz(hpv_handle h, int which, const double* planes, size_t n);

/* The norm the variational residual is measured in, for the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D, with or without
 * hpv_set_nonlinear / hpv_set_trainable / hpv_set_ansatz).  kind 0 (the default) is  loss_e = mean over the active functions of R^2,
 * the Euclidean norm of the residual's coordinates in the basis phi_n = P_{n+1} - P_{n-1}, which is far from orthonormal.  kind 1 is
 * the dual norm of the element's discrete test space (robust VPINNs),
 *     loss_e = R_e^T G_e^{-1} R_e,      G_e the Gram matrix of the element's ACTIVE test functions in  (grad v, grad w) + mass (v, w),
 * not divided by their count; lossv = sum_e loss_e as before.  For kappa = 1, beta = sigma = 0 it is the squared H^1 seminorm (mass 0)
 * of the Galerkin projection of the error onto the element's bubble space; for the other operators it is equivalent to that up to
 * the continuity and inf-sup constants.  G_e^{-1} is applied through the tensor structure: with K, M the 1-D stiffness and mass
 * matrices of n functions on the reference interval and K S = M S Lambda, S^T M S = I,
 *     G_e^{-1} = (S_y (x) S_x) diag(1 / d) (S_y (x) S_x)^T,      d[a][b] = (Jy/Jx) lam_x[b] + (Jx/Jy) lam_y[a] + mass Jx Jy
 * on half widths Jx, Jy (1-D: d[b] = lam_x[b] / Jx + mass Jx).  The caller hands the pairs over for EVERY count 1 .. nt (per-element
 * counts use the leading block, and S of n functions is not a sub-block of S of n + 1): Sx = [ntx][ntx][ntx], entry [n - 1] the
 * n x n matrix in its leading block, zero-padded; lamx = [ntx][ntx]; Sy, lamy the same for nty, NULL in 1-D.  Everything is copied.
 * The _dual instantiations of k_project_lin | _nl | _id (csrc/hpv_dual_norm.h) run in the same launch slot; hpv_get_residuals keeps
 * returning the raw R; d lossv / d c_m, the data and the flux term are unchanged; with hpv_set_strong_form, column 0 of
 * hpv_linear_indicators is the element's dual-norm loss (columns 1 - 4 stay on the raw R).  hpv_kernel_variant appends ";dual".
 * The tables belong to the test-function tables: hpv_set_tables drops them, and every pass then returns -3 until this call is
 * repeated or kind 0 is given -- a handle that had the dual norm never silently trains the other loss.  kind 0 restores the plain
 * handle bit for bit.  Side effects: waits for the handle's stream and drops the captured iteration graphs, like hpv_set_nonlinear.
 * The setting is not state: hpv_get_state / hpv_set_state do not carry it.
 * Returns 0; -3 for a handle of another problem or scheme and before hpv_set_tables; -1 (the handle keeps what it had) for an unknown
 * kind, mass < 0 or not finite, missing tables, a non-finite entry, an eigenvalue <= 0 inside a count's block, and an element whose
 * dual-norm kernel would need more than 64 KiB of LDS (the scratch is appended where the integrand region cannot hold it); -2 on a
 * HIP error.
 * Out of scope: the other problem classes and the whole-iteration kernels, non-symmetric optimal test norms, the data and flux terms,
 * gathering indicators across GPUs.  Gram matrices of a weighted (kappa) inner product and of mapped elements: hpv_set_residual_gram. */
int hpv_set_residual_norm(hpv_handle h, int kind, double mass, const double* Sx, const double* lamx, const double* Sy, const double* lamy);

/* The same dual norm through one DENSE inverse Gram factor per owned element (kind 2), for the inner products whose Gram matrix is no
 * Kronecker sum: the physical H^1 product of a mapped element (hpv_set_element_points) and the energy product
 * (sym(K) grad v, grad w) + mass (v, w) of a variable or full-tensor kappa.  The caller factors G_e = L_e L_e^T of each element's ACTIVE
 * test functions once (hp_vpinns_amd/quadrature.py: gram_factors, a Gauss-Legendre rule of the Gram matrix's own) and hands over
 * W_e = L_e^{-1}: W is [n_owned][NR][NR], NR = ntx*nty, row-major in the full index k*ntx + r of R[k][r], lower triangular, exactly zero
 * in the rows and columns of inactive functions.  Then
 *     loss_e = |W_e R_e|^2 = R_e^T G_e^{-1} R_e          d loss_e / d R = 2 W_e^T (W_e R_e)
 * in the _dense instantiations of k_project_lin | _nl | _id, with and without the tensor operator (csrc/hpv_dual_dense.h: one
 * workgroup per element, W_e read in place twice per pass, no atomics, the same bits from call to call), in the launch slot of
 * kind 1.  It follows the contract of hpv_set_residual_norm: linear problems and the variational scheme only; 1-D, 2-D and mapped
 * handles; everything is copied; it waits for the handle's stream and drops the captured iteration graphs; it replaces kind 1 if
 * that was set (and hpv_set_residual_norm(h, 1, ..) replaces it); hpv_set_residual_norm(h, 0, ..) removes it and restores the plain
 * handle bit for bit.  hpv_kernel_variant appends ";dual=dense"; hpv_get_residuals keeps returning the raw R; with
 * hpv_set_strong_form on boxes, column 0 of hpv_linear_indicators is the dense dual loss.  The setting is not state.
 * The factors belong to the elements, their counts and the test-function tables: hpv_set_tables, hpv_set_elements,
 * hpv_set_element_boxes, hpv_set_element_points and hpv_set_active_tests* drop them, and every pass then returns -3 until this call
 * is repeated or kind 0 is given -- a handle that had a dual norm never silently trains mean(R^2).  On mapped handles kind 1 stays
 * refused and hpv_set_element_points stays refused while kind 1 is set; while kind 2 is set it is accepted and drops the factors.
 * Returns 0; -3 for a handle of another problem or scheme and before hpv_set_tables / the elements; -1 (the handle keeps what it
 * had) for an element whose kernel would need more than 64 KiB of LDS (y = W_e R_e, NR doubles, is appended where the integrand
 * region cannot hold it), a wrong n, NULL, a non-finite entry, a non-zero entry above the diagonal or in an inactive row or column,
 * a diagonal entry <= 0 on an active index; -2 on a HIP error.
 * Out of scope: the other problem classes and the whole-iteration kernels, non-symmetric optimal test norms, the data and flux terms,
 * a Gram matrix that follows a trainable coefficient, gathering indicators across GPUs. */
#define HPV_NORM_DUAL_DENSE 2
int hpv_set_residual_gram(hpv_handle h, const double* W, size_t n);
int hpv_backend_in_use(hpv_handle h);                       /* HPV_BACKEND_GENERIC or HPV_BACKEND_MFMA */
/* Launch structure of the most recent reverse-mode pass over the quadrature batch (tests assert that the kernel they mean to
 * exercise is the one that ran): 0 separate forward / projection / reverse launches, 1 forward + projection-fused reverse,
 * 2 element-resident whole-iteration kernel (Poisson-2D var_form 1 on 20x20-, 16x16-, 12x12- or 10x10-point elements with up to
 * 10x10 / 8x8 / 6x6 / 5x5 test functions), 3 the same in SPLIT mode (small shards),
 * 4 whole-iteration tile kernel (small elements of the other channel sets), 5 whole-iteration kernel for few tall elements
 * (80x80 points: many workgroups per element exchange partial residual sums), 6 the generic element-resident whole-iteration
 * kernel (any instantiated tensor-product element shape, e.g. 16x16 / 8x8; several tiles per wave); -1 before the first such pass. */
int hpv_pass_structure(hpv_handle h);
/* The kernel INSTANTIATION(s) of that pass by name, e.g. "k_iter_fused<L=3,SPLIT=false,QT=true>" (quarter-tile plan) vs
 * "k_iter_fused<L=3,SPLIT=false,QT=false>" (7/6/6/6 whole tiles: HPV_NO_QUARTER_TILE=1, or the build's AGPR guard tripped),
 * "k_iter_tall<..,QT=true> split=32", "k_iter_tile<..>", "k_fwd_mfma<..> + k_project_tp<20x20/10x10> + k_bwd_mfma<..>",
 * "k_mlp_fwd_generic + k_project<..> + k_mlp_bwd_generic"; a strong-form pass (HPV_SCHEME_PINN) reports the layer kernels of its
 * collocation batch, "k_fwd_wide<..> + k_pinn_residual + k_bwd_wide<..>" (not the value-only pair that the boundary / data batch runs
 * beside it, in either scheme) -- so that a green test run says which code it exercised. */
int hpv_kernel_variant(hpv_handle h, char* buf, size_t n);
/* How this library was built: "k_iter_fused=ok|no-quarter-tile|absent;k_iter_tall=ok|no-quarter-tile|absent;test_hooks=0|1"
 * (csrc/build.sh compiles a whole-iteration kernel out when the compiler's registers reach its hand-managed AGPR range;
 * test_hooks=1 only in libhpvpinn_testhooks.so, the build that carries the fault-injection knobs of the tests). */
const char* hpv_build_info(void);
/* 1 when hpv_step / hpv_step_record replay captured iteration hipGraphs, 0 when they launch eagerly (HPV_NO_GRAPH=1, a foreign
 * stream, or a collective that refused stream capture -- hpv_step then drops to eager launches instead of failing). */
int hpv_graphs_in_use(hpv_handle h);
/* Number of parameter updates applied through this handle since hpv_create (synchronises).  After hpv_step returned -7 (an
 * in-kernel exchange between the workgroups of one element timed out) the difference to the value before the call says how many
 * of the requested iterations took place. */
int hpv_updates_applied(hpv_handle h, long long* n);
/* on = 0: from now on only launch structures without an in-kernel exchange (no SPLIT mode, no k_iter_tall: what HPV_FUSE=s
 * selects at creation); on = 1 allows them again.  Drops captured iteration graphs.  hpv_step / hpv_step_record call it
 * themselves when such an exchange timed out (-7 inside), and finish the requested iterations on the remaining structures:
 * the run continues instead of ending on a shared GPU (connected ranks all do so in the same call: the failure travels with
 * the all-reduced buffer).  They return -7 instead when HPV_EXCHANGE_FALLBACK=0 is set.
 * hpv_shared_element_kernels: the current setting (0 after such a fallback). */
int hpv_shared_element_kernels(hpv_handle h);
int hpv_set_shared_element_kernels(hpv_handle h, int on);
/* N_quad is a free hyper-parameter (P1:237, P2:282, P3:47); the element-resident kernels are instantiated for a few rules and
 * take a SMALLER rule padded with zero-weight points (exact: the tables are w * phi).  Whether that pays depends on the problem, the
 * shard and the device, so the library decides, with the plan its own dispatch follows: for problem `pde` in variational form
 * `var_form` under a network of n_hidden hidden layers, the widest max_width neurons, and a shard of n_elem_shard elements with q
 * points per direction and ntx x nty test functions (1-D: nty ignored) on `device` (its CU count; 256 when no device can be queried),
 * *q_dev = the rule to hand to hpv_set_quadrature (== q: leave the rule alone) and *nt_dev = the test-function count to hand to
 * hpv_set_tables in 1-D (the 80-point kernel takes 60 functions and per-element counts; == ntx otherwise).  A rule is padded only
 * where an element-resident kernel of this build takes that form, network and rule and ONE WORKGROUP PER ELEMENT will run -- not
 * where the element loop or the separate launches take the grid (on many rounds the padded points cost more than the structure
 * saves).  No handle needed; < 0: bad arguments (an unknown pde / var_form pair among them). */
int hpv_rule_advice(int device, int pde, int var_form, int n_hidden, int max_width, int q, int ntx, int nty, long n_elem_shard, int* q_dev, int* nt_dev);
/* How the whole-iteration kernel takes a shard of n_elem_shard elements of one of its 2-D rules (q = 12, 16, 20 points per
 * direction; N_el_x, N_el_y are free: P2:282-283, P3:44-45) under a network of n_hidden hidden layers on `device`: 0 = not at all
 * (the separate launches), 1 = one workgroup per element, 2 = the element loop (CUs workgroups walk the elements), 3 = the full
 * rounds with one workgroup per element + the ragged tail (n mod CUs elements) shared by 2 - 8 workgroups each in a second launch.
 * The dispatch's own plan (csrc/hpv_mfma.h, hpv_fused_plan_shard) with this build's instantiations; < 0: bad arguments. */
int hpv_grid_plan(int device, int q, int n_hidden, long n_elem_shard);
/* The network value and its input-derivative channels at the owned quadrature points, [C][n_owned*qx*qy]
 * (channel order: u, then d/dx, d/dy (d/dt), then the second derivatives the variational form integrates) --
 * what net_u / net_du / net_dxu / net_dyu / net_dtu return (P1:140-148, P2:171-185, P3:232-245).  One forward launch. */
int hpv_eval_channels(hpv_handle h, double* out, size_t n);
/* Test hook: the device activation s(x), s'(x) (cfg.act) and the ROCm math library's s(x) for the same
 * inputs, so tests can bound the error of the hand-written fp64 tanh (replaces tf.tanh, P2:165). */
int hpv_debug_activation(hpv_handle h, const double* x, int n, double* a, double* a1, double* ref);
/* Average device time (ms) per launch of kernel class `which` since the last reset, measured with
 * hipEvents on the handle's stream when timing is enabled; which: 0 mlp_fwd, 1 project, 2 mlp_bwd. */
int hpv_enable_timing(hpv_handle h, int on);
int hpv_kernel_time_ms(hpv_handle h, int which, double* avg_ms, long* launches);
/* Average duration (ms) of the whole-iteration kernel -- forward, projection and reverse pass of the shard in ONE launch (the work of
 * P2:98-132 on the quadrature batch) -- over `reps` back-to-back launches bracketed by ONE hipEvent pair on the handle's stream: the
 * per-launch timers above carry ~3.5 us of event overhead per pair, this one amortises it (it still contains the gaps between the
 * launches).  Parameters, moments and the packed buffer of the last pass are left as they are (no finalize, no update).  -4 when the
 * handle's iteration is not one such launch (separate launches, an in-kernel exchange between workgroups, strong-form branch). */
int hpv_time_iteration_kernel(hpv_handle h, int reps, double* avg_ms);

/* Stand-alone launch of the per-element projection (residual + adjoint) kernel on synthetic
 * integrand channels already resident on the device -- the HBM-roofline measurement of
 * SURVEY.md section 8(d).  n_elem elements of the handle's (qx,qy,ntx,nty) shape; returns the
 * average kernel time over `reps` launches. */
int hpv_bench_projection(hpv_handle h, long n_elem, int reps, double* avg_ms, double* bytes_per_launch);
/* Same with the adjoint half switchable: do_adjoint = 0 is the residual-only launch whose algorithmic bytes are
 * SURVEY.md 8(d)'s 8 (C_u N + 2 N_R) (read the integrated channels and F, write R). */
int hpv_bench_residual(hpv_handle h, long n_elem, int reps, int do_adjoint, double* avg_ms, double* bytes_per_launch);
/* One such launch on the same seeded synthetic data, condensed to checksums {sum R, sum R^2, sum loss_e, sum |gbar|, sum gbar^2,
 * sum_e (e mod 97) loss_e}: lets tests compare the kernel plans that serve large batches (streaming / column-in-registers)
 * with each other and with the general projection kernel on the SAME data. */
int hpv_bench_residual_checksums(hpv_handle h, long n_elem, int do_adjoint, double* sums6);

#ifdef __cplusplus
}
#endif
#endif /* HPVPINN_H */
