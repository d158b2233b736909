/* symode.h -- C ABI of libsymode_hip.so: the MI355X (gfx950) SINDy hot path.
 *
 * The reference (Rose-STL-Lab/symmetry-ode-discovery) has no FFI boundary: the hot path is
 * Python calling torch ops.  Each entry point below replaces the torch-op sequence named in
 * its comment (file:line of the reference) and is what a binding for that sequence would
 * call (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (fp32 unless stated), row-major,
 *     contiguous; nothing is allocated or freed inside the library;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued asynchronously on it, no call synchronises;
 *   - return value: 0 = ok, < 0 = SYMODE_E_* argument error (nothing was launched),
 *     > 0 = a hipError_t reported by the launch;
 *   - `flags`: bit 0 = include_sine, bit 1 = include_exp (reference sindy.py:74-77);
 *   - library column order: [1 | x_i | x_i x_j (i<=j) | (x_i x_j) x_k (i<=j<=k) | ... |
 *     sin x_i | exp x_i]  (reference sindy.py:7-30, 68-77); orders 4-5 continue the nesting.
 *   - batched entry points take `n_problems` independent (trajectory, seed) problems laid
 *     out back to back: x[s] = x + s*n*d, xi[s] = xi + s*d*p, ...
 */
#ifndef SYMODE_H
#define SYMODE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYMODE_FLAG_SINE 1
#define SYMODE_FLAG_EXP 2

#define SYMODE_OK 0
#define SYMODE_E_UNSUPPORTED (-1) /* (d, order, flags) outside the compiled library set */
#define SYMODE_E_NULLPTR (-2)
#define SYMODE_E_BADSIZE (-3)
#define SYMODE_E_WORKSPACE (-4) /* workspace missing or too small */
#define SYMODE_E_ALIGN (-5)     /* pointer not 4-byte (fp32) / 8-byte (fp64) aligned */

/* ABI version of this header (bumped on any signature change). */
int symode_abi_version(void);

/* The optional SYMODE_* tuning / A-B variables are read once, when the library is first used; this
 * reads them again (tests and tuning tools that compare two settings inside one process).  No reference counterpart. */
void symode_reload_env(void);
const char* symode_error_string(int code);

/* p = number of library columns; SYMODE_E_UNSUPPORTED if (d, order, flags) is not compiled in.
 * replaces: SINDyRegression.get_term_num, sindy.py:179-189 */
int symode_lib_size(int d, int order, int flags);

/* Bytes of scratch the batched reductions need for (n_problems, n) at this library.
 * The same buffer serves symode_loss_grad / symode_aug_gram / the symreg entry points. */
size_t symode_workspace_bytes(int d, int order, int flags, long n_problems, long n);

/* One-time preparation of a freshly allocated workspace (enqueued on `stream`): writes the header the
 * one-launch reductions keep their "last workgroup done" tickets in.  The tickets reset themselves, so one
 * call per allocation is enough; a workspace that never saw this call makes the reductions return NaN
 * (never stale numbers).  A workspace must not be shared by calls that run concurrently on different streams.
 * replaces: nothing in the reference (its reductions are torch ops); it exists so that the closure body
 * train.py:663-664 + 689 is ONE kernel launch at the 50x2500x2 shape. */
int symode_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* Theta(x) materialised: theta_out (n, p).
 * replaces: SINDyRegression.eval_Theta_at, sindy.py:201-203 (term functions sindy.py:7-30) */
int symode_theta(const float* x, long n, int d, int order, int flags, float* theta_out, void* stream);

/* out (n, d) = Theta(x) @ (xi * mask)^T ; mask may be NULL (all ones). xi, mask: (d, p).
 * replaces: SINDyRegression.forward, sindy.py:79-82 */
int symode_forward(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask,
                   float* out, void* stream);

/* Fused Theta-build + residual + MSE + gradient, never materialising Theta:
 *   r = Theta(x) (xi*mask)^T - dx ;  loss[s] = inv_count * sum r^2 ;
 *   grad[s] (d, p) = 2 * inv_count * (r^T Theta) * mask.
 * inv_count = 1/(n*d) gives torch's MSELoss mean; a rank holding a shard passes
 * 1/(n_global*d) and all-reduces (SUM) loss and grad.
 * replaces: closure body train.py:663-664 + backward train.py:689 (and 789-790, 802). */
int symode_loss_grad(const float* x, const float* dx, long n_problems, long n, int d, int order, int flags,
                     const float* xi, const float* mask, float inv_count, float* loss_out, float* grad_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* K explicit Euler steps x <- x + dt * Theta(x)(xi*mask)^T, out (n, d).
 * replaces: odeint(regressor, x, t, dt, 'euler'), model_utils.py:233-238 (n_steps = int(t/dt)
 * is computed by the caller). method: 0 = euler, 1 = rk4 (model_utils.py:241-247). */
int symode_odeint(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask,
                  int n_steps, float dt, int method, float* out, void* stream);

/* Same integration, every intermediate state kept: traj (n_steps, n, d), traj[s] = state after step s+1.
 * replaces: odeint(regressor, x0, t, dt, method, full_traj=True), model_utils.py:249-254 -- the long-term
 * prediction roll-out of evaluation/eval_ltp.py:31-37 (n_steps sequential Theta builds + GEMMs there). */
int symode_odeint_traj(const float* x, long n, int d, int order, int flags, const float* xi, const float* mask,
                       int n_steps, float dt, int method, float* traj, void* stream);

/* Roll-out error of n_models models on n_ics held-out trajectories, ONE launch, the predicted trajectories never stored.
 * x_true (n_ics, n_steps + 1, d) fp32 contiguous: the layout the data sets hold before flattening; the integration
 * starts from x_true[:, 0].  xi, mask: (n_models, d, p), mask may be NULL.  method as symode_odeint; one thread per
 * (model, trajectory) runs the steps of symode_odeint_traj and after step k forms
 *     e = mean_j (x_true[i, k+1, j] - x_pred[j])^2        (fp32: each difference and square rounded, no FMA, the squares
 *                                                          summed over j in index order, times 1/d -- for d <= 2 bit for bit
 *                                                          torch's ((x - xp) ** 2).mean(-1); at d = 3 torch adds the three
 *                                                          squares in another order and may differ in the last place)
 *   err_out (n_models, n_ics, n_steps) fp32 = e; may be NULL (nothing is written then);
 *   mean_err_out (n_models, n_ics) fp64 = the fp32 e values added in step order in fp64, over n_steps: NaN / inf when the
 *                model diverges (no early exit, inf / NaN propagate as in the per-model path);
 *   horizon_out (n_models, n_ics) int32 = number of leading steps with e <= bound (false for NaN); bound = +inf counts
 *                the leading finite steps; horizon == n_steps: the bound was never exceeded.
 * No workspace, no atomics: the outputs are bit-deterministic.  n_ics == 0 or n_models == 0: nothing to do (0).
 * replaces: eval_ltp_accuracy called once per model, evaluation/eval_ltp.py:31-43 (roll-out model_utils.py:241-254,
 * error eval_ltp.py:43), for every model of a seed sweep at once. */
int symode_rollout_error(const float* x_true, long n_ics, int n_steps, int d, int order, int flags, const float* xi,
                         const float* mask, long n_models, float dt, int method, float bound, float* err_out,
                         double* mean_err_out, int* horizon_out, void* stream);

/* Augmented Gram matrix in fp64 (MFMA f64): A = [Theta(x) | dx] (n, p+d),
 *   gram_out[s] (p+d, p+d) = A^T A   (row-major, both triangles filled).
 * Every quantity of the ridge-augmented least-squares solve (sindy.py:261-288) and of the
 * MSE closure is a function of this matrix; x is fixed for a whole run (train.py:626).
 * replaces: the normal-equation content of solve_SINDy_one_step, sindy.py:250-315. */
int symode_aug_gram(const float* x, const float* dx, long n_problems, long n, int d, int order, int flags,
                    double* gram_out, void* workspace, size_t workspace_bytes, void* stream);

/* Same, for n_problems index subsets of ONE shared data set: problem s uses the m points
 * x[idx[s*m + i]], i < m (int32 row indices < n_src; the caller guarantees the range).
 * replaces: the per-seed DataLoader subsample (main.py:36-38) of a seed sweep
 * (the run_scripts seed loops, `for i in {0..49}`) followed by sindy.py:261-288, for all seeds at once. */
int symode_aug_gram_gather(const float* x, const float* dx, long n_src, const int* idx, long n_problems, long m, int d,
                           int order, int flags, double* gram_out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Weak SINDy: the contraction of the test functions with the library, fused with the library build (fp64 MFMA, Theta
 * never written).  x (n_t, d): ONE trajectory on a uniform time grid; V, V_drv (n_test, n_t) fp32 row-major: the test
 * functions and their derivatives times dt (sindy.py:346-347).  out: fp64 row-major (R, C) with R = 16*ceil(2 n_test/16),
 * C = 16*ceil((p+d)/16):
 *     out[k, j]            = sum_t V[k, t] Theta_j(x_t)          k < n_test, j < p        (= G, sindy.py:363)
 *     out[n_test + k, p+i] = -sum_t V_drv[k, t] x_i(t)           k < n_test, i < d        (= b, sindy.py:364)
 * (the other entries are by-products of the 16x16 tiles).  n_test <= 128.
 * replaces: self.V @ self.regressor.eval_Theta_at(x) and -self.V_drv @ x, sindy.py:362-364. */
int symode_weak_gram(const float* x, long n_t, int d, int order, int flags, const float* V, const float* V_drv, int n_test,
                     double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Weak SINDy for the seeds of a sweep at once: every seed reads one window of ONE shared data set, and everything its
 * fit needs is the (p+d, p+d) normal matrix of the window,
 *     N = Z^T M Z,   Z = [G | b] (n_test, p+d),   G = V Theta(x_window),   b = -V_drv x_window,
 * whose blocks N[:p, :p] = G^T M G and N[:p, p:] = G^T M b are the system of sindy.py:365-370.
 * x (n_ics, n_steps, d) fp32: the data set; windows (n_windows, 2) int32 ON THE DEVICE, row s = [trajectory, start]:
 * window s is rows start .. start + n_t - 1 of that trajectory.  V, V_drv (n_test, n_t) fp32 as for symode_weak_gram,
 * M (n_test, n_test) fp64 (= V V^T, sindy.py:348).  n_test <= 128, p <= 64, d <= 4, n_t <= n_steps, n_windows <= 65535.
 *     aug_out (n_windows, p+d, p+d) fp64 row-major, both triangles, exactly symmetric: the layout symode_aug_gram
 *             leaves, so symode_stlsq_sweep and symode_host_stlsq_sweep take it as it is (ridge gamma = sqrt(w_sindy_reg));
 *     z_out   NULL, or (n_windows, R, C) fp64 with R, C of symode_weak_gram: window s holds, bit for bit, what
 *             symode_weak_gram writes for x[trajectory, start : start + n_t];
 *     bad_out (n_windows) int32: 1 for a row outside trajectory in [0, n_ics), start in [0, n_steps - n_t] -- such a
 *             window reads nothing from x and its matrices are all zero -- else 0.  The kernel checks the row before it
 *             forms an address from it.
 * Two launches (window contraction on the fp64 matrix cores, then a workgroup per window for the sums and N), fixed
 * summation order, no atomics: equal inputs give equal bytes.  The workspace holds n_windows * R/16 * C/16 * gx tiles of
 * 256 doubles behind its header, gx = min(64, ceil(n_t / 256)); symode_weak_gram uses the same gx unless its workspace
 * is short.
 * replaces: the window draw and slice of main_wsindy.py:24-29 + sindy.py:362-370, for all seeds of a run-script loop
 * (`for i in {0..49}; do python main_wsindy.py --seed $i`) at once. */
int symode_weak_normal_windows(const float* x, long n_ics, long n_steps, int d, int order, int flags,
                               const int* windows, long n_windows, long n_t,
                               const float* V, const float* V_drv, int n_test, const double* M,
                               double* aug_out, double* z_out, int* bad_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* S1, linear-latent symmetry regulariser (train.py:502-507 with the intended [1]):
 *   loss = sum_v sum_n || Xi_m J_Theta(z_n)(L_v z_n) - L_v Xi_m Theta(z_n) ||^2,
 *   grad (d, p) = dloss/dxi (masked).  L: (n_gen, d, d). */
int symode_symreg_linear(const float* z, long n, int d, int order, int flags, const float* xi, const float* mask,
                         const float* L, int n_gen, float* loss_out, float* grad_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The entries of the reversed symmetry closure (this one, _batched, symode_loss_grad_reversed, the two _constj forms and
 * their _live forms) are ONE implementation behind seven signatures: the same argument checks in the same order, one grid rule, one
 * launcher.  They differ only in whether dx joins (the fused closure, which also keeps more workgroups on one large
 * problem), whether jgx is the compact table (_constj), and in n_g = 0, which the materialised regulariser alone accepts.
 *
 * S4, reversed symmetry regulariser with (g(x), J_g(x)) precomputed once
 * (model_utils.py:126-170; g and J_g do not depend on xi, model_utils.py:172-211):
 *   loss = sum_g mean_{n,j} ( J_g(x_n) h(x_n) - h(g(x_n)) )^2,  h = Theta(.)(xi*mask)^T,
 *   grad (d, p) = dloss/dxi (masked).  gx: (n_g, n, d), jgx: (n_g, n, d, d). */
int symode_symreg_reversed(const float* x, const float* gx, const float* jgx, int n_g, long n, int d, int order,
                           int flags, const float* xi, const float* mask, float* loss_out, float* grad_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same regulariser for n_problems independent (trajectory, seed) problems in ONE launch:
 * x (S, n, d), gx (S, n_g, n, d), jgx (S, n_g, n, d, d), xi / mask (S, d, p); loss (S), grad (S, d, p).
 * inv_count as in symode_loss_grad (1/(n*d) for the plain mean; a rank holding a point shard passes 1/(n_global*d)
 * and all-reduces).  replaces: the per-seed processes of run_scripts/lv_noise99_eq_rreg.sh, each evaluating
 * model_utils.py:160-168 per closure. */
int symode_symreg_reversed_batched(const float* x, const float* gx, const float* jgx, int n_g, long n_problems, long n, int d,
                                   int order, int flags, const float* xi, const float* mask, float inv_count,
                                   float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* The whole closure of the reversed-regulariser fit in ONE pass over the points: the residual shares Theta(x) and
 * h(x) with the regulariser and x is read once (40 instead of 16 + 32 bytes per point at d = 2, n_g = 1):
 *     loss2_out[s] = inv_count * ( sum r^2 , sum_g sum u^2 ),   r = h(x) - dx,  u = J_g(x) h(x) - h(g(x)),
 *     grad_out[s]  = d( loss2[0] + w_sym * loss2[1] ) / dxi   (masked).
 * Layouts as in symode_symreg_reversed_batched; n_g >= 1.
 * replaces: train.py:663-664 + 675-679 + 689 with sym_reg_type 'r' (loss_sindy_x + w_sym_reg * symm_loss, backward). */
int symode_loss_grad_reversed(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_problems, long n,
                              int d, int order, int flags, const float* xi, const float* mask, float inv_count, float w_sym,
                              float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* The whole closure of the LATENT fit in one pass over the points.  With the autoencoder frozen (eval mode, not among
 * the optimiser's variables) z = enc(x), dz = J_enc(x) dx and A_n = J_dec(z_n) are data; a thin QR A_n = Q_n B_n turns
 * |A_n h - dx_n|^2 into |B_n h - y_n|^2 + const with y_n = Q_n^T dx_n (B = A, y = dx when the observed and the latent
 * dimension agree):
 *     loss2_out[s] = inv_count * ( sum r_z^2 , sum r_x^2 ),   r_z = h(z) - dz,  r_x = B h(z) - y,  h = Theta(.)(xi*mask)^T,
 *     grad_out[s]  = d( loss2[0] + w_pair * loss2[1] ) / dxi   (masked);  w_pair = 0 still produces loss2[1].
 * z, dz, y (S, n, d); B (S, n, d, d) row-major; xi / mask (S, d, p); loss2 (S, 2), grad (S, d, p).  inv_count, the
 * workspace (symode_workspace_bytes / _init) and the argument checks as in symode_loss_grad_reversed.
 * replaces: train.py:647-661 + 689 (--use_latent: autoencoder forward, compute_dz, compute_dx, the two MSE terms and
 * their backward, per closure). */
int symode_loss_grad_latent(const float* z, const float* dz, const float* B, const float* y, long n_problems, long n, int d,
                            int order, int flags, const float* xi, const float* mask, float inv_count, float w_pair,
                            float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* Is J_g(x) the same matrix at every point of each (problem, group element)?  One streaming pass over
 * jgx (S, n_g, n, d, d), run once per data set: every point's matrix is compared BITWISE (as 32-bit words) with point 0
 * of its own (s, g) slab -- -0.0 differs from +0.0, a NaN anywhere answers "no" -- and different slabs may hold
 * different matrices.  table_out (S, n_g, d, d) fp32 = the matrix of point 0 of every slab (always written);
 * flag_out: ONE int32 on the device = 1 if every slab is constant, else 0 (the caller reads it back; no call synchronises).
 * d in 1..4 (library independent), n_g >= 1.  True for any linear or affine group action on the observed coordinates and
 * for a frozen linear autoencoder; then the _constj entries below replace their materialised counterparts.
 * replaces: nothing in the reference -- precompute_symmreg_r, model_utils.py:172-211, stores vmap(jacfwd(.)) per point
 * whatever the map is. */
int symode_jacobian_constant(const float* jgx, int n_g, long n_problems, long n, int d, float* table_out, int* flag_out,
                             void* stream);

/* symode_symreg_reversed_batched on a point-constant Jacobian: jgx is the compact (S, n_g, d, d) table of
 * symode_jacobian_constant, nothing of J_g is streamed (8 + 8 n_g instead of 8 + 24 n_g bytes per point at d = 2).
 * Every other argument, the workspace and the result as there -- bit-identical to that entry on the materialised
 * (S, n_g, n, d, d) copies of the table; n_g >= 1.
 * replaces: model_utils.py:160-168 per closure, as symode_symreg_reversed_batched. */
int symode_symreg_reversed_batched_constj(const float* x, const float* gx, const float* jgx, int n_g, long n_problems, long n,
                                          int d, int order, int flags, const float* xi, const float* mask, float inv_count,
                                          float* loss_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                          void* stream);

/* symode_loss_grad_reversed on a point-constant Jacobian: jgx is the compact (S, n_g, d, d) table (24 instead of 40
 * bytes per point at d = 2, n_g = 1).  Every other argument, the workspace and the result as there -- bit-identical to
 * that entry on the materialised copies of the table; n_g >= 1.
 * replaces: train.py:663-664 + 675-679 + 689 with sym_reg_type 'r', as symode_loss_grad_reversed. */
int symode_loss_grad_reversed_constj(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_problems,
                                     long n, int d, int order, int flags, const float* xi, const float* mask, float inv_count,
                                     float w_sym, float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* The two _constj entries for coefficients whose zero columns are known beforehand: live_columns is a set of library
 * columns, bit k set = column k may hold a coefficient in some equation row (p > 64: pass all ones).  An equivariance
 * constraint keeps whole columns of xi at zero for the length of a fit -- for the planar rotations every even degree --
 * up to the round-off of its basis Q; the caller that knows the set (CoefMap.live_columns) says so here.  Contract:
 *   - coefficients in columns outside the set are treated as zero, whatever xi holds there;
 *   - the gradient in those columns is returned as zero;
 *   - every other result is, on an xi that IS zero outside the set, bit-identical to the plain _constj entry;
 *   - a set the library has no kernel for (anything not inside "constant column + odd degrees" of the d = 2 plain
 *     polynomial libraries of order 4-5; all ones; SYMODE_CLOSURE_LIVE=0) runs the dense kernel on xi as it is: the
 *     results of the plain _constj entry.
 * The kernels for a set leave out the per-point work of the dead columns (order 5: 13 of 21 columns stay).
 * Arguments, checks and workspace as in the plain entries; added to ABI version 8 (nothing existing changed). */
int symode_symreg_reversed_batched_constj_live(const float* x, const float* gx, const float* jgx, int n_g, long n_problems,
                                               long n, int d, int order, int flags, const float* xi, const float* mask,
                                               unsigned long long live_columns, float inv_count, float* loss_out,
                                               float* grad_out, void* workspace, size_t workspace_bytes, void* stream);
int symode_loss_grad_reversed_constj_live(const float* x, const float* dx, const float* gx, const float* jgx, int n_g,
                                          long n_problems, long n, int d, int order, int flags, const float* xi,
                                          const float* mask, unsigned long long live_columns, float inv_count, float w_sym,
                                          float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes,
                                          void* stream);

/* Is g(x) the linear image J x of x under the compact table?  x (S, n, d), gx (S, n_g, n, d), table (S, n_g, d, d) as
 * symode_jacobian_constant left it.  flag_out (one int32, device): 1 when, for every component a of every point,
 *     | gx_a - sum_b J_ab x_b |  <=  4 u sum_b |J_ab| |x_b|,   u = 2^-24,
 * evaluated in fp64 on the fp32 inputs (any fp32 evaluation of the dot product lies within about 2 u of the sum), and x, gx
 * and the table are finite; else 0 -- a NaN or an infinity anywhere, an offset (affine actions are not linear), any other map.
 * m_out (S, n_g, p, p) fp64: the substitution matrix M of each (problem, group element), Theta(J x) = M Theta(x), built in
 * fp64 from the fp32 table, rows and columns in the library's column order, block diagonal by degree (exact zeros outside
 * the blocks); meaningful where the flag is 1.  One streaming pass, meant to run once per data set.
 * d = 2, flags = 0, order 1-5, n_g = 1; anything else: SYMODE_E_UNSUPPORTED.  Added to ABI version 8 (nothing existing
 * changed).
 * replaces: nothing in the reference (precompute_symmreg_r, model_utils.py:172-211, stores g(x) per point whatever g is). */
int symode_linear_action(const float* x, const float* gx, const float* table, int n_g, long n_problems, long n, int d, int order,
                         int flags, double* m_out, int* flag_out, void* stream);

/* symode_loss_grad_reversed_constj_live under a linear action (symode_linear_action answered 1; m_table is its m_out).
 * With h = Xi Theta:  u = J h(x) - h(J x) = C Theta(x), C = J Xi - Xi M (fp64 products, once per problem and launch), and
 * sum_n u Theta(J x)^T = (sum_n u Theta(x)^T) M^T: the point loop reads x and dx alone (16 instead of 24 bytes per point),
 * evaluates the library once and applies [Xi; C] to it; the gradient is R + w_sym (J^T U - U M^T), formed before the partial
 * rows.  Results: those of the _constj_live entry on gx = J x exactly, up to rounding -- NOT bit-identical (gx is not read;
 * u comes from C instead of the difference of two fp32 chains, which is the more accurate where u is round-off).
 * Where the launcher's table keeps the streamed kernels for the library and column set, and everywhere with
 * SYMODE_CLOSURE_FOLD=0, the call IS the _constj_live entry on (gx, table), bit for bit.  The body taken is left in word 1 of
 * the workspace header.  Workspace as for the other closures.  d = 2, flags = 0, order 1-5, n_g = 1; anything else:
 * SYMODE_E_UNSUPPORTED.  Added to ABI version 8 (nothing existing changed). */
int symode_loss_grad_reversed_linear(const float* x, const float* dx, const float* gx, const float* table, const double* m_table,
                                     int n_g, long n_problems, long n, int d, int order, int flags, const float* xi,
                                     const float* mask, unsigned long long live_columns, float inv_count, float w_sym,
                                     float* loss2_out, float* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* symode_loss_grad_reversed_linear with the regulariser taken from the library's Gram matrix instead of the points.
 * g_table (S, 1, p, p) fp64: G = sum_n Theta(x_n) Theta(x_n)^T of each problem over the n points of THIS call, RAW sums (no
 * inv_count) -- the top-left p x p block of symode_aug_gram on the same x.  A function of x alone: build it once per data
 * set.  Then  sum_n |u_n|^2 = sum_j c_j G c_j^T  and  U = sum_n u_n Theta^T = C G,  so the point loop carries the residual
 * alone (Theta, h = Xi Theta, r, sum r^2, R: fp32, the bits of the _linear entry's kernel on the same grid) and ONE workgroup
 * per problem forms C, U, the value and (J - I)^T U - U (M - I)^T in fp64 and adds them to its fp64 partial row.
 * loss2_out[:, 0] is bit-identical to the _linear entry's; loss2_out[:, 1] and the regulariser's share of the gradient agree
 * with it up to rounding (they are the more accurate: fp64 against fp32 sums over the points).  The term is linear in G:
 * shards of points add.  Where the launcher's table keeps the plain fold kernel for the library and column set, and
 * everywhere with SYMODE_FOLD_GRAM=0, the call IS symode_loss_grad_reversed_linear, bit for bit (SYMODE_FOLD_GRAM=2: the
 * Gram form for every fold library, for tests).  The form taken is left in word 1 of the workspace header (bit 64).
 * Refuses what the _linear entry refuses, and a null (SYMODE_E_NULLPTR) or misaligned (SYMODE_E_ALIGN) g_table.
 * Added to ABI version 8 (nothing existing changed). */
int symode_loss_grad_reversed_linear_gram(const float* x, const float* dx, const float* gx, const float* table,
                                          const double* m_table, const double* g_table, int n_g, long n_problems, long n, int d,
                                          int order, int flags, const float* xi, const float* mask,
                                          unsigned long long live_columns, float inv_count, float w_sym, float* loss2_out,
                                          float* grad_out, void* workspace, size_t workspace_bytes, void* stream);

/* symode_loss_grad_reversed_linear_gram with the residual, too, taken from a matrix built once: no pass over the points.
 * aug_table (S, p+d, p+d) fp64: symode_aug_gram of each problem's x, dx, RAW sums, [Gtt Gty; Gty^T Gyy]; a function of x and dx
 * alone.  With W = xi * mask (columns outside live_columns count as 0):
 *     sum_n |W Theta_n - dx_n|^2 = tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy),     sum_n r_n Theta_n^T = W Gtt - Gty^T,
 * and the regulariser from Gtt, m_table and table (S, 1, d, d) by the statements of the _linear_gram entry's kernel.  fp64
 * throughout, one rounding to fp32 per output; one wave per problem, one launch.  x, dx and gx are not read.
 * Outputs: loss2_out (S, 2) = (mse, regulariser), grad_out (S, d, p) = d(mse + w_sym regulariser)/dxi, masked, zero outside
 * live_columns; loss_out (S) = mse + w_sym regulariser (may be NULL).  inv_count is a double here.
 * The coefficient map in the same launch: with q (d p, r) fp32 given, xi must be NULL and Xi = reshape(q beta) + const:
 * beta (S, r) with rows beta_stride floats apart (>= r); flat = q beta in fp64, viewed as (d, p) (use_kron != 0) or as the transposed (p, d) view; const_ (S, d), rows
 * const_stride floats apart (>= d), or NULL is added to column 0; ONE rounding to fp32, from where on the call is the call on that xi (written to xi_out (S, d, p)
 * when not NULL).  Then also g_beta_out (S, r) = vec(grad) q in the same view and g_const_out (S, d) = grad[:, :, 0] (or
 * NULL), both from the fp64 gradient, rounded once.  Without q: beta, const_, xi_out, g_beta_out, g_const_out must be NULL.
 * The shards of a point-sharded problem add: every output but xi_out is linear in aug_table.
 * workspace: an initialised one (symode_workspace_init); only its header is used -- word 1 gets what the fold kernel of the
 * same column set leaves there, in its Gram form, plus bit 128.
 * d = 2, flags = 0, order 1-5, n_g = 1; anything else, and every call under SYMODE_CLOSURE_FOLD=0, SYMODE_FOLD_GRAM=0 or
 * SYMODE_FOLD_RESID_GRAM=0 (the caller keeps the entries with a point loop): SYMODE_E_UNSUPPORTED.  r outside [1, d p]:
 * SYMODE_E_BADSIZE.  Added to ABI version 8 (nothing existing changed).
 * replaces: the closure body train.py:663-664 + 675-679 + 689 with get_Xi (sindy.py:169-176) and its transpose. */
int symode_loss_grad_reversed_linear_quad(const double* aug_table, const double* m_table, const float* table, int n_g, long n_problems,
                                          int d, int order, int flags, const float* xi, const float* q, const float* beta,
                                          long beta_stride, const float* const_, long const_stride, int r, int use_kron,
                                          const float* mask,
                                          unsigned long long live_columns, double inv_count, float w_sym, float* loss2_out,
                                          float* loss_out, float* grad_out, float* xi_out, float* g_beta_out, float* g_const_out,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* symode_loss_grad_reversed_linear_quad with the map, reduced ONCE to a quadratic form in the fit's own variables.  For fixed
 * aug_table, m_table, table, q, mask, live_columns and w_sym that entry's loss is an exact quadratic in z = (beta, const),
 * K = r + d_c numbers per problem (d_c = 2 with has_const, else 0).  With P z = view(q beta) + const on column 0 (masked, dead
 * columns 0) and g(W) the gradient by xi that entry forms at coefficients W (no rounding of W to fp32 here):
 *     column i of H = 1/2 P^T (g(P e_i) - g(0)),   h = -1/2 P^T g(0),   c0 = inv_count tr(Gyy),
 *     b_out[s] = 1/2 (B + B^T),  B = [[H, -h], [-h^T, c0]]   (K+1, K+1) fp64, row-major, (S, K+1, K+1) in all,
 * so that with v = [z; 1]:  loss = v^T B v  and  d loss / d z = 2 (B v)[:K].  fp64 throughout; one wave per problem walks the
 * K + 1 states; a set-up step, to be repeated when any operand changes.  mask (S, 2, p) fp32 or NULL.
 * order 1-5 (d = 2, plain polynomial library, one group element); other orders, and every call under SYMODE_QUAD_REDUCED=0 or a
 * switch that refuses symode_loss_grad_reversed_linear_quad: SYMODE_E_UNSUPPORTED.  r outside [1, 2 p] or K + 1 > 16:
 * SYMODE_E_BADSIZE.  No workspace.  Added to ABI version 8 (nothing existing changed).
 * replaces: nothing in the reference; the fixed-data part of the closure body train.py:663-689, formed once per fit. */
int symode_quad_reduce(const double* aug_table, const double* m_table, const float* table, long n_problems, int order,
                       const float* q, int r, int use_kron, int has_const, unsigned long long live_columns, double inv_count,
                       float w_sym, const float* mask, double* b_out, void* stream);

/* The step on the reduced form: b (S, K+1, K+1) fp64 of symode_quad_reduce, k = K, d_c = 0 or the number of constants;
 * beta (S, K - d_c) fp32 with rows beta_stride floats apart (>= K - d_c), const_ (S, d_c) with rows const_stride floats apart
 * (>= d_c; NULL, with g_const_out, when d_c = 0).  loss_out (S) = v^T B v, g_beta_out (S, K - d_c) and g_const_out (S, d_c) =
 * 2 (B v)[:K], each formed in fp64 and rounded to fp32 once.  A group of 16 lanes per problem, no shared memory; reads
 * 8 (K+1)^2 bytes per problem.  Xi, the loss pair and the gradient by Xi are not formed.
 * workspace: an initialised one (symode_workspace_init); only its header is used -- word 1 gets what
 * symode_loss_grad_reversed_linear_quad leaves there for the same order and live_columns, plus bit 256.
 * K + 1 > 16, k < 1, d_c outside [0, k), a stride below its row: SYMODE_E_BADSIZE; switches and orders as symode_quad_reduce.
 * Added to ABI version 8 (nothing existing changed).
 * replaces: the closure body train.py:663-664 + 675-679 + 689 with get_Xi (sindy.py:169-176) and its transpose. */
int symode_quad_step(const double* b, long n_problems, int k, int d_c, int order, unsigned long long live_columns,
                     const float* beta, long beta_stride, const float* const_, long const_stride, float* loss_out,
                     float* g_beta_out, float* g_const_out, void* workspace, size_t workspace_bytes, void* stream);

/* Gram matrix of the reversed regulariser: for S problems (layouts as in symode_symreg_reversed_batched, n_g >= 1)
 *     gram_out[s] (d p, d p) fp64 = sum_g sum_n B^T B,   B[i, (j, a)] = J_g(x_n)[i, j] theta_a(x_n) - delta_ij theta_a(g x_n),
 * rows and columns in Xi's (d, p) row-major order, both triangles filled: the regulariser of symode_symreg_reversed_batched
 * is inv_count * v^T R v with v = vec(xi * mask).  RAW sums (no inv_count): shards and chunks of points simply add.
 * Exact fp64 products of the fp32 library, fp64 sums.  The workspace is its own (symode_symreg_reversed_gram_workspace_bytes;
 * no symode_workspace_init needed).  SYMODE_E_UNSUPPORTED for libraries with d p > 88.
 * replaces: nothing in the reference; the fixed-data part of model_utils.py:160-168, accumulated once per fit. */
size_t symode_symreg_reversed_gram_workspace_bytes(int d, int order, int flags, int n_g, long n_problems, long n);
int symode_symreg_reversed_gram(const float* x, const float* gx, const float* jgx, int n_g, long n_problems, long n, int d,
                                int order, int flags, double* gram_out, void* workspace, size_t workspace_bytes, void* stream);

/* Same, for n_problems index subsets of ONE shared data set: x (n_src, d), gx (n_g, n_src, d), jgx (n_g, n_src, d, d) fp32;
 * problem s uses the m rows idx[s*m + k], k < m (int32 row indices < n_src; the caller guarantees the range).
 * gram_out[s] (d p, d p) is bit-identical to symode_symreg_reversed_gram on the materialised copies x[idx[s]],
 * gx[:, idx[s]], jgx[:, idx[s]]: the same item order (g m + k), grid and fixed-order finalize.  The workspace query returns
 * 0 where the library is not supported (d p > 88).
 * replaces: the per-seed processes of run_scripts/lv_noise99_eq_rreg.sh and selkov_noise20_eq_symreg3.sh, each pushing its
 * own subsample through model_utils.py:160-168; g(x) and J_g(x) of a fixed LaLiGAN are computed once for all seeds. */
size_t symode_symreg_reversed_gram_gather_workspace_bytes(int d, int order, int flags, int n_g, long n_problems, long m);
int symode_symreg_reversed_gram_gather(const float* x, const float* gx, const float* jgx, int n_g, long n_src, const int* idx,
                                       long n_problems, long m, int d, int order, int flags, double* gram_out, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* The closure of the non-latent fit as a quadratic form of fixed fp64 matrices, for S problems (library independent,
 * d p <= 256): aug_gram (S, p+d, p+d) from symode_aug_gram, rev_gram (S, d p, d p) from symode_symreg_reversed_gram or NULL;
 * xi, mask (S, d, p) fp32 (mask may be NULL = ones), W = xi * mask, v = vec(W):
 *     mse = inv_count (tr(W Gtt W^T) - 2 tr(W Gty) + tr(Gyy)),   reg = inv_count v^T R v.
 * rev_gram == NULL: loss_out (S) = mse, grad_out (S, d, p) = d mse / dxi (masked), as symode_loss_grad;
 * else loss_out (S, 2) = (mse, reg) and grad_out = d(mse + w_sym reg)/dxi (masked), as symode_loss_grad_reversed.
 * fp64 arithmetic, one rounding to fp32.  One launch, one wave per problem, no workspace.
 * replaces: the closure body train.py:663-664 (+ 675-679 with sym_reg_type 'r') + 689, on the data of train.py:626-629. */
int symode_quad_closure(const double* aug_gram, const double* rev_gram, long n_problems, int d, int p, const float* xi,
                        const float* mask, double inv_count, float w_sym, float* loss_out, float* grad_out, void* stream);

/* Reverse mode of symode_forward, given g = dL/d(out) (n, d):
 *   grad_x (n, d) = J_Theta(x)^T (xi*mask)^T g   (skipped when grad_x is NULL),
 *   grad_xi (d, p) = (g^T Theta(x)) * mask.
 * replaces: autograd's backward through sindy.py:79-82 (cat-of-products + matmul). */
int symode_vjp(const float* x, const float* g, long n, int d, int order, int flags, const float* xi, const float* mask,
               float* grad_x, float* grad_xi, void* workspace, size_t workspace_bytes, void* stream);

/* Forward mode: out (n, d) = Theta(x)(xi*mask)^T (skipped when out is NULL) and
 *   jv (n, d) = (J_Theta(x) v)(xi*mask)^T  for tangents v (n, d).
 * replaces: torch.autograd.functional.jvp(regressor, x, v)[1], the double-backward trick of
 * model_utils.py:56, 166 and train.py:505. */
int symode_forward_jvp(const float* x, const float* v, long n, int d, int order, int flags, const float* xi,
                       const float* mask, float* out, float* jv, void* stream);

/* Reverse mode of symode_forward_jvp, given g_out = dL/d(out) (may be NULL = 0) and g_jv = dL/d(jv):
 *   grad_x (n, d) (includes the second-order term through J_Theta(x) v), grad_v (n, d),
 *   grad_xi (d, p) = (g_out^T Theta + g_jv^T (J_Theta v)) * mask.
 * replaces: the backward of the create_graph=True jvp in model_utils.py:32, 56 (what makes the
 * reference need a twice-differentiable regressor). */
int symode_jvp_vjp(const float* x, const float* v, const float* g_out, const float* g_jv, long n, int d, int order,
                   int flags, const float* xi, const float* mask, float* grad_x, float* grad_v, float* grad_xi,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Offline data generation: n_traj RK4 orbits of dx/dt = Theta(x) xi^T (xi (d, p) fp64, unmasked) from x0
 * (n_traj, d) fp64, n_steps of size dt; every `subsample`-th state and its exact derivative are written as
 * fp32 x_out, dx_out (n_traj, ceil(n_steps/subsample), d).  One trajectory per thread, fp64 arithmetic.
 * replaces: solve_ode_batch + the subsample/transposes of gen_data, data_utils/ode.py:7-28, 45-48, for systems
 * the library can express (all four shipped ones: evaluation/eval_eq.py:88-105). */
int symode_rk4_traj(const double* x0, long n_traj, int d, int order, int flags, const double* xi, int n_steps, double dt,
                    int subsample, float* x_out, float* dx_out, void* stream);

/* Seed sweeps: idx_out (n_seeds, m) int32, rows ascending -- for every seed the m-subset of range(n) holding the m
 * smallest of n counter-based keys key(seed, row) (a 32-bit bijective mix of the row under two words derived from the
 * seed): a seed's subsample depends on that seed alone (not on the other seeds,
 * the world size or the device).  seeds: n_seeds int64 on the device.  One workgroup per seed (radix select + ordered
 * compaction).  The table is what symode_aug_gram_gather takes.
 * replaces: the first batch of DataLoader(train_dataset, batch_size=int(len * lbfgs_subsample), shuffle=True) of each
 * seed's process, main.py:36-38 (there: torch's generator, one process per seed). */
int symode_seeded_subsamples(long n, long m, const long long* seeds, int n_seeds, int* idx_out, void* stream);

/* Fused K-step Euler flow f and its tangent map: x_out = f(x), t_out = J_f(x) v  for
 * f = n_steps explicit Euler steps of dx/dt = Theta(x)(xi*mask)^T (all steps in registers).
 * replaces: forward_step = odeint(regressor, ., int_t, int_dt) and jvp(forward_step, x, v_x)[1] of the
 * infinitesimal symmetry regulariser, train.py:669-673 + model_utils.py:56. */
int symode_euler_jvp(const float* x, const float* v, long n, int d, int order, int flags, const float* xi,
                     const float* mask, int n_steps, float dt, float* x_out, float* t_out, void* stream);

/* Reverse mode of symode_euler_jvp, given g_x = dL/d(x_out), g_t = dL/d(t_out):
 * grad_x = dL/dx, grad_v = dL/dv (n, d), grad_xi (d, p) masked.  Step states are recomputed from (x, v).
 * replaces: autograd's double-backward through n_steps regressor calls (model_utils.py:32, 56). */
int symode_euler_jvp_vjp(const float* x, const float* v, const float* g_x, const float* g_t, long n, int d, int order,
                         int flags, const float* xi, const float* mask, int n_steps, float dt, float* grad_x,
                         float* grad_v, float* grad_xi, void* workspace, size_t workspace_bytes, void* stream);

/* L-BFGS search direction d = -H g (two-loop recursion) for n_problems independent problems of n <= 256
 * parameters: curvature pairs in ring buffers old_dirs / old_stps (S, history, n), ro (S, history), with
 * per-problem `head` (oldest slot) and `count` (pairs stored), int64; h_diag (S) scales the initial Hessian.
 * replaces: the history loops of torch.optim.LBFGS.step that train.py:630-695 runs per seed and per
 * inner iteration (new: the reference sweeps seeds as separate processes). */
int symode_lbfgs_direction(const float* g, const float* old_dirs, const float* old_stps, const float* ro,
                           const long* head, const long* count, const float* h_diag, long n_problems, int n,
                           int history, float* d_out, void* stream);

/* Self-test hook: every lane's wave-wide sum of in (n_waves * 64 floats) by the shuffle butterfly and by the
 * permlane-swap / DPP form the L-BFGS kernels use; the two must agree bit for bit (tests/test_gpu_kernels.py). */
int symode_selftest_wave_sum(const float* in, float* butterfly_out, float* dpp_out, long n_waves, void* stream);

/* One launch for everything torch.optim.LBFGS.step (no line search) does between two closure evaluations, one wavefront
 * per problem.  The launch takes the closure's new_loss (S) / new_g (S, n) into loss / g (l1 != 0: as the bare data term,
 * objective w_x * data + w_reg * |params|_1 over the raw parameters, train.py:680-688, gradient w_x * g + w_reg *
 * sign(params), formed here) and then, by `mode`:
 *   SYMODE_LBFGS_BEGIN   opens an optimiser step: every problem whose frozen[s] == 0 (frozen == NULL: every problem) runs
 *                        torch's optimality test max|g| <= tol_grad and, unless it holds, the first iteration; frozen
 *                        problems get act = 0 and are otherwise left untouched.
 *   SYMODE_LBFGS_ACCEPT  finishes the running iteration of the problems with act != 0: the three stopping tests of
 *                        torch/optim/lbfgs.py (max|g| <= tol_grad, max|t d| <= tol_change, |loss - prev_loss| < tol_change);
 *                        those still active go straight into the next iteration.  frozen is not read.
 * An iteration is: curvature-pair update of the ring buffers, two-loop recursion, step length (first iteration: min(1,
 * 1/|g|_1) lr), directional-derivative test, move x += t d.  State arrays as in symode_lbfgs_direction plus n_iter (S)
 * int64, d / prev_g (S, n), t / prev_loss (S); act (S) bytes out: the problem moved (its closure must be re-evaluated).
 * An optimiser step of max_iter iterations is  closure, BEGIN, (closure, ACCEPT) x (max_iter - 1).  Any other mode:
 * SYMODE_E_BADSIZE.
 * replaces: the body of torch.optim.LBFGS.step that train.py:630-695 runs per seed and per inner iteration. */
#define SYMODE_LBFGS_ACCEPT 1
#define SYMODE_LBFGS_BEGIN 2
int symode_lbfgs_step(int mode, const float* new_loss, const float* new_g, const unsigned char* frozen, float tol_grad, int l1,
                      float w_x, float w_reg, float* params, float* g, float* loss, unsigned char* act, long* n_iter, float* d,
                      float* t, float* old_dirs, float* old_stps, float* ro, long* head, long* count, float* h_diag,
                      float* prev_g, float* prev_loss, long n_problems, int n, int history, float lr, float tol_change,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Device-resident L-BFGS trainer: train_SIGED_lbfgs for n_problems independent problems with NOTHING on the host between
 * two epochs.  An epoch is
 *     closure, BEGIN-update, (closure, ACCEPT-update) x (max_iter - 1), epoch-end
 * -- 2 max_iter + 1 launches.  The closure is one of three, named by the descriptor's `closure`:
 *     SYMODE_CLOSURE_STREAM  symode_loss_grad, or symode_loss_grad_reversed when n_g > 0 (one pass over the points),
 *     SYMODE_CLOSURE_GRAM    symode_quad_closure (the quadratic form of matrices built once; no point data),
 *     SYMODE_CLOSURE_LATENT  symode_loss_grad_latent (the latent fit on operands computed once).
 * The update launches are the kernel of symode_lbfgs_step (same two modes) extended by the coefficient map of the equivariance
 * constraint (Xi = reshape(Q beta) + const and its chain rule, sindy.py:169-176, formed inside the launch), and the
 * epoch-end launch is the per-epoch logic of train.py:697-725: NaN guard, the two update norms, convergence- / period-
 * triggered thresholding (strict >, monotone, sindy.py:192-195) with optimiser reset, twice-converged stop.  Every epoch
 * leaves one record per problem in `log` (and, with log_detail, the coefficients and mask after the epoch's events), which
 * may be pinned host memory: the host reads it after synchronising on the epoch and produces the reference's prints,
 * wandb record and checkpoints from it.
 * replaces: train.py:630-725 (torch.optim.LBFGS.step + the epoch logic), per seed. */
#define SYMODE_CLOSURE_STREAM 0 /* symode_loss_grad, or symode_loss_grad_reversed when n_g > 0 */
#define SYMODE_CLOSURE_GRAM 1   /* symode_quad_closure on aug_gram / rev_gram */
#define SYMODE_CLOSURE_LATENT 2 /* symode_loss_grad_latent */
typedef struct symode_trainer {
    /* closure data, read only: S = n_problems problems back to back */
    const float* x;            /* (S, n_points, d) */
    const float* dx;           /* (S, n_points, d) */
    const float* gx;           /* (S, n_g, n_points, d) reversed-regulariser operands; n_g == 0: not read (plain MSE) */
    const float* jgx;          /* (S, n_g, n_points, d, d) */
    int n_g;
    float w_sym;               /* regulariser weight relative to the MSE: data term = mse + w_sym * regulariser */
    long n_problems, n_points;
    int d, order, flags;
    float inv_count;           /* 1 / (points over all ranks * d) */
    void* workspace;           /* reduction scratch of the closure kernel (symode_workspace_bytes / _init) */
    size_t workspace_bytes;
    /* parametrisation */
    const float* q_eff;        /* (d p, r) row-major: Q with rows in Xi's (d, p) order; NULL = unconstrained (params are Xi) */
    int r;                     /* columns of Q */
    int allow_constant;        /* const is added to column 0 of Xi (sindy.py:173-175) */
    int n_params;              /* d p, or r + d under the constraint */
    /* objective  w_x * data + w_reg * |params|_1  (l1 != 0) and torch.optim.LBFGS's settings */
    float w_x, w_reg;
    int l1;
    float lr, tol_grad, tol_change;
    int max_iter, history;
    /* epoch logic (train.py:697-725) */
    float threshold, tol_update, near_band;
    int st_freq;
    /* state: ONE device allocation of symode_trainer_layout(...) bytes, prepared by symode_trainer_init */
    void* state;
    size_t state_bytes;
    /* per-epoch records, ring of log_epochs epochs (device-visible memory; pinned host memory allowed):
     *   log        (log_epochs, S, 8): [event code, mse, regulariser, |params|_1 of the last closure, update norm,
     *              update norm vs the last convergence, near-threshold coefficients at this event, epoch]
     *              event code: 0 none, 1 threshold on convergence, 2 threshold on st_freq, 3 final convergence, 4 NaN,
     *              -1 problem already finished
     *   log_test   (log_epochs, S, 2): closure value at the epoch's final coefficients and mask (train.py:739-751), written
     *              by symode_trainer_run(..., test_eval != 0)
     *   log_xi, log_mask (log_epochs, S, d p) and log_params (log_epochs, S, n_params), or all NULL: coefficients, mask and
     *              parameters after the epoch's events */
    float* log;
    float* log_test;
    float* log_xi;
    float* log_mask;
    float* log_params;
    int log_epochs;
    /* Gram-form closure (SYMODE_CLOSURE_GRAM): with aug_gram (S, p+d, p+d) fp64 every closure of the trainer is the
     * quadratic form of these matrices at inv_count / w_sym, and x, dx, gx, jgx and workspace may be NULL; rev_gram
     * (S, d p, d p) fp64 or NULL adds the reversed regulariser (then the closure is the (mse, regulariser) pair). */
    const double* aug_gram;
    const double* rev_gram;
    /* Which closure every evaluation of this trainer is (SYMODE_CLOSURE_*).  The kind alone decides: what it needs is
     * checked before anything is launched, and pointers that belong to another kind are never read.
     *   STREAM  symode_loss_grad on x, dx (workspace), or symode_loss_grad_reversed on x, dx, gx, jgx when n_g > 0 (then
     *           the closure is the (mse, regulariser) pair);
     *   GRAM    symode_quad_closure on aug_gram (/ rev_gram: the pair), see above;
     *   LATENT  symode_loss_grad_latent on x := z, dx := dz, latent_B, latent_y (workspace); always the pair
     *           (loss_sindy_z, loss2[1]).  w_sym is the weight of loss2[1] in the loss VALUE; the closure itself is launched
     *           with w_pair = 0, so the gradient is the z-term's alone -- as in the reference, whose compute_dx
     *           (autoencoder.py:106-108) is a functional jvp without create_graph: its result is cut from the graph, so
     *           loss_sindy_x is logged and added but never differentiated. */
    int closure;
    const float* latent_B;     /* (S, n_points, d, d) */
    const float* latent_y;     /* (S, n_points, d) */
} symode_trainer;

#define SYMODE_TRAINER_FIELDS 29
/* Byte offsets of the state block's arrays (offsets_out[SYMODE_TRAINER_FIELDS], may be NULL) and its total size.  Order:
 * params, xi, mask, cl_loss (S, 2), cl_grad (S, d p), g, loss, act (u8), n_iter (i64), d, t, old_dirs, old_stps, ro, head
 * (i64), count (i64), h_diag, prev_g, prev_loss, prev, pprev, n_iters (i32), done (u8), nan (u8), finished (u8), epochs
 * (i32), near (i32), l1_last, test_grad (S, d p); fp32 unless stated.  Unconstrained problems keep ONE array for params and xi.  cl_loss and
 * cl_grad are adjacent: a sharded run sums [cl_loss | cl_grad] over the ranks between closure and update. */
size_t symode_trainer_layout(long n_problems, int n_params, int dp, int history, int constrained, size_t* offsets_out);

/* Prepare the state block: zero it, h_diag = 1, params = prev = pprev = params0 (S, n_params), mask = mask0 (S, d p; NULL =
 * ones), xi from params.  params0 / mask0 may be host or device pointers (copied with hipMemcpyAsync). */
int symode_trainer_init(const symode_trainer* T, const float* params0, const float* mask0, void* stream);

/* The three launches of an epoch on their own (a sharded run all-reduces [cl_loss | cl_grad] between closure and update).
 * symode_trainer_closure: loss_out / grad_out NULL = the state's cl_loss / cl_grad.  symode_trainer_update: mode
 * SYMODE_LBFGS_BEGIN (first iteration of an optimiser step) or SYMODE_LBFGS_ACCEPT (all later ones), as symode_lbfgs_step. */
int symode_trainer_closure(const symode_trainer* T, float* loss_out, float* grad_out, void* stream);
int symode_trainer_update(const symode_trainer* T, int mode, void* stream);
int symode_trainer_epoch_end(const symode_trainer* T, int epoch, void* stream);

/* n_epochs whole epochs starting at epoch0, enqueued back to back; test_eval != 0 adds one closure launch per epoch into
 * log_test.  Problems that finished earlier cost empty launches only. */
int symode_trainer_run(const symode_trainer* T, int epoch0, int n_epochs, int test_eval, void* stream);

/* A hyper-parameter grid on shared Gram matrices: the Gram-form trainer with a per-problem table.  A grid point changes only
 * four numbers around the fixed matrices of symode_quad_closure -- step size, L1 weight, threshold, weight of R against G --
 * so n_problems = grid points x seeds problems fit from n_sets = seeds sets of matrices: problem s reads set s % n_sets and
 * row s of hyper wherever the launch-wide scalar of symode_trainer stood (lr: the step length, first iteration included;
 * w_reg: L1 value and gradient, 0 for every problem when base.l1 == 0; threshold: thresholding event and near count, near_band
 * stays launch-wide; w_sym: the pair's weight in loss value and gradient, not read without rev_gram).  One wave per problem
 * in every launch and no arithmetic shared between problems: problem s is bit for bit the one-problem scalar trainer on set
 * s % n_sets at row s's values.  State block, symode_trainer_layout and symode_trainer_init are the scalar trainer's, on
 * &G->base.  The four entries are symode_trainer_closure / _update / _epoch_end / _run with the table; each refuses, before
 * anything is launched: G, hyper or aug_gram NULL (SYMODE_E_NULLPTR); base.closure != SYMODE_CLOSURE_GRAM, n_sets < 1 or
 * n_problems % n_sets != 0 (SYMODE_E_BADSIZE); hyper not 16-byte aligned (SYMODE_E_ALIGN); then whatever the scalar entry
 * refuses, with its code.
 * replaces: one sweep of a run script per value of --lr_sindy / --w_sindy_reg / --threshold / --w_sym_reg (new: the
 * reference has no hyper-parameter search; every value is a loop of per-seed processes). */
#define SYMODE_TRAINER_HYPER 4          /* columns of hyper: lr, w_reg, threshold, w_sym */
typedef struct symode_trainer_grid {
    symode_trainer base;   /* closure must be SYMODE_CLOSURE_GRAM; n_problems counts ALL problems (grid points x seeds);
                              its lr, w_reg, threshold and w_sym are not read */
    const float* hyper;    /* (n_problems, SYMODE_TRAINER_HYPER) fp32, device memory, 16-byte aligned */
    long n_sets;           /* aug_gram is (n_sets, p+d, p+d), rev_gram (n_sets, d p, d p) or NULL;
                              problem s reads set s % n_sets */
} symode_trainer_grid;
int symode_trainer_grid_closure(const symode_trainer_grid* G, float* loss_out, float* grad_out, void* stream);
int symode_trainer_grid_update(const symode_trainer_grid* G, int mode, void* stream);
int symode_trainer_grid_epoch_end(const symode_trainer_grid* G, int epoch, void* stream);
int symode_trainer_grid_run(const symode_trainer_grid* G, int epoch0, int n_epochs, int test_eval, void* stream);

/* symode_quad_closure for n_problems problems on n_sets sets of matrices (n_problems % n_sets == 0, else SYMODE_E_BADSIZE):
 * problem s reads aug_gram[s % n_sets] (and rev_gram[s % n_sets]) and, with rev_gram, takes w_sym from column 3 of row s of
 * hyper (n_problems, SYMODE_TRAINER_HYPER) fp32; without rev_gram the table is not read.  Outputs as symode_quad_closure.
 * replaces: the closure of symode_quad_closure, once per grid point. */
int symode_quad_closure_grid(const double* aug_gram, const double* rev_gram, long n_sets, long n_problems, int d, int p,
                             const float* xi, const float* mask, double inv_count, const float* hyper /* (n_problems, 4) */,
                             float* loss_out, float* grad_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Device-resident minibatch Adam trainer: n_epochs whole epochs of train_SIGED's plain branch (no latent space, no symmetry
 * regulariser) for n_problems independent problems in ONE launch, one workgroup per problem, nothing on the host inside.
 * A step takes the rows idx[epoch, problem, step, :] of the shared (n_src, d) arrays x / dx -- an entry outside [0, n_src)
 * is padding: it is not read and does not count in the batch's divisor, -1 is the canonical pad (a short last batch) --
 * and does   loss = w_x * sum r^2 / (valid rows * d) + w_reg * |params|_1 (l1 != 0),  backward,  torch.optim.Adam.step
 * (m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, t += 1, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)).
 * The parameters are Xi (q_eff NULL, n_params = d p) or [beta | const] with Xi = reshape(q_eff beta) + const in column 0
 * (q_eff (d p, r), allow_constant, n_params = r + d: the conventions of symode_trainer); the L1 term is over the raw
 * parameters whatever the mask says.  After every epoch e (global number epoch0 + e) with st_freq > 0 and
 * (epoch + 1) % st_freq == 0:  mask &= |Xi| > threshold (strict, monotone).  A batch of padding alone is no step.  A
 * problem whose batch loss is not finite stops there: the step that meets such a loss is not taken, the state stays as that
 * step found it, and step[s] becomes -t - 1 (t = steps taken); such a problem is left alone by every later launch.  The
 * loss is the only thing tested: a finite loss whose gradient or second moment overflows still takes its step and may
 * write non-finite parameters, which the NEXT step's loss then reveals -- the frozen state is the one that step found.  Every sum runs in an order fixed by the
 * row's position in the batch: two launches on the same inputs agree bit for bit, and so does a fit cut into launches.
 *   idx     (n_epochs, n_idx_problems, n_steps, batch) int32; n_idx_problems = 1: all problems share the table
 *   params, m, v (n_problems, n_params), step (n_problems) int32, mask (n_problems, d p): state, read and written back
 *   xi_out  (n_problems, d p): Xi (unmasked) after the launch
 *   log     (n_epochs, n_problems, 8): [mean batch MSE over the epoch's steps, mean |params|_1 (as the loss saw it), steps
 *           taken, coefficients with mask set within near_band of the threshold at this epoch's event, 1 = frozen (NaN),
 *           1 = thresholding event, epoch, 0]
 *           An epoch in which the problem takes no step (every batch padding alone, or the problem frozen) has no mean:
 *           columns 0 and 1 hold NaN (0 / 0) and column 2 holds 0; the thresholding event of a problem that is not frozen
 *           still takes place.
 * n_epochs == 0 or n_problems == 0: nothing to do.  n_params and d p are at most 256.
 * replaces: train.py:491-547 (the per-minibatch loop of train_SIGED and its epoch end) plus torch.optim.Adam.step. */
int symode_adam_epochs(const float* x, const float* dx, long n_src, const int* idx, long n_idx_problems, int n_epochs,
                       int n_steps, int batch, long n_problems, int d, int order, int flags, const float* q_eff, int r,
                       int allow_constant, int n_params, float lr, float beta1, float beta2, float eps, float w_x, float w_reg,
                       int l1, float threshold, int st_freq, int epoch0, float near_band, float* params, float* m, float* v,
                       int* step, float* mask, float* xi_out, float* log, void* stream);

/* symode_adam_epochs with the reversed symmetry regulariser (EquivSINDy-r) in every minibatch loss:
 *   loss = w_x * sum_b |h(x_b) - dx_b|^2 / (valid rows * d)
 *        + w_sym * sum_g sum_b |J_g(x_b) h(x_b) - h(g x_b)|^2 / (valid rows * d) + w_reg * |params|_1,   h(y) = Theta(y) (Xi * mask)^T,
 * on operands computed once per data set (they depend neither on Xi nor on the problem), shared by all problems:
 *   gx      (n_g, n_src, d)     g(x) of every source row, per group element
 *   jgx     (n_g, n_src, d, d)  J_g(x), jgx[g, i, a, b] = d g(x_i)_a / d x_b
 * A valid entry i of idx reads x[i], dx[i], gx[:, i] and jgx[:, i]; a padding entry (outside [0, n_src)) reads none of the
 * four arrays and does not count.  Every other argument, the state, the freezing rule (applied to MSE + regulariser) and
 * the fixed order of every sum are those of symode_adam_epochs; log column 7 is the mean over the epoch's steps of the batch
 * regulariser (unweighted, the value train.py logs as loss_sym_reg; NaN like columns 0 and 1 for an epoch without a step
 * when n_g > 0).  n_g == 0 (gx, jgx may be NULL) computes what
 * symode_adam_epochs computes, bit for bit, and writes 0 into column 7.  The regulariser's gradient is accumulated at
 * weight w_sym / w_x next to the residual's, so n_g > 0 with w_x <= 0 (or NaN) is refused with SYMODE_E_BADSIZE; n_g < 0 too.
 * replaces: train.py:491-547 with loss_sym_reg = symmreg_r (model_utils.py:160-168, the JVP as the explicit matvec on the
 * operands of model_utils.py:172-211) plus torch.optim.Adam.step. */
int symode_adam_epochs_reversed(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_src,
                                const int* idx, long n_idx_problems, int n_epochs, int n_steps, int batch, long n_problems,
                                int d, int order, int flags, const float* q_eff, int r, int allow_constant, int n_params,
                                float lr, float beta1, float beta2, float eps, float w_x, float w_reg, float w_sym, int l1,
                                float threshold, int st_freq, int epoch0, float near_band, float* params, float* m, float* v,
                                int* step, float* mask, float* xi_out, float* log, void* stream);

/* symode_adam_epochs on the --use_latent branch of train_SIGED under a frozen autoencoder (the optimiser steps the SINDy
 * coefficients alone, so the autoencoder is data): per-row operands computed once per fit (model_utils.latent_operands),
 * shared by all problems and gathered by the row numbers of idx,
 *   z, dz   (n_src, d)      z = enc(x), dz = J_enc(x) dx
 *   B       (n_src, d, d)   the decoder's Jacobian at z reduced by a thin QR, J_dec(z_b) = Q_b B_b
 *   y       (n_src, d)      Q_b^T dx_b
 *   e       (n_src)         |dx_b - Q_b y_b|^2; read only when D_obs > d (D_obs == d: every e_b is 0, e may be NULL)
 *   L       (n_gen, d, d)   the generators L_g (v[:d, :d] of generator.get_full_basis_list()), read uniformly
 * With W = Xi * mask, rows = the valid entries of the batch and, per valid row b, theta = Theta(z_b), h = W theta:
 *   r_z = h - dz_b,   r_x = B_b h - y_b,   and for every generator   dtheta = J_Theta(z_b)(L_g z_b),   u = W dtheta - L_g h
 *   mse_z = sum_b |r_z|^2 / (rows d)
 *   mse_x = (sum_b |r_x|^2 + sum_b e_b) / (rows D_obs)
 *   sym   = sum_g sum_b |u|^2                       NOT divided by rows (torch.norm(..)**2)
 *   loss  = w_z mse_z + w_x mse_x + w_sym sym + w_reg |params|_1
 *   dloss/dXi = mask * [ (2 w_z / (rows d)) sum_b r_z theta^T + 2 w_sym sum_g sum_b ( u dtheta^T - (L_g^T u) theta^T ) ]
 *               (+ the L1 sign term on params)
 * mse_x contributes NO gradient: compute_dx is a functional jvp without create_graph, so train.py adds and logs the term but
 * it is cut from the graph (the same fact as SYMODE_CLOSURE_LATENT).  The Adam step, the coefficient map, padding entries
 * (none of the five arrays is read, the entry does not count), a batch of padding alone, thresholding, the near count, the
 * freezing rule -- applied to w_z mse_z + w_x mse_x + w_sym sym -- and the fixed order of every sum are those of
 * symode_adam_epochs.  With n_gen == 0, B = I, y = dz and D_obs == d the entry leaves in params, m, v and mask what
 * symode_adam_epochs leaves on (z, dz) with its w_x = w_z, bit for bit.
 *   log     (n_epochs, n_problems, SYMODE_ADAM_LOG_LATENT = 10): columns 0-6 as symode_adam_epochs with column 0 = mean mse_x,
 *           7 = mean sym, 8 = mean mse_z (all unweighted; NaN for an epoch without a step), 9 = 0
 * Refused with SYMODE_E_BADSIZE beyond the checks of symode_adam_epochs: n_gen < 0, w_z <= 0 or NaN (the regulariser's
 * gradient is accumulated at weight w_sym / w_z, and without w_z no data term reaches the coefficients), D_obs < d,
 * e == NULL with D_obs > d, L == NULL with n_gen > 0.
 * replaces: train.py:491-508, 522-547 (the use_latent branch of the per-minibatch loop: encoder pass, compute_dz, compute_dx,
 * the linear-latent regulariser and the epoch end) plus torch.optim.Adam.step. */
#define SYMODE_ADAM_LOG_LATENT 10
int symode_adam_epochs_latent(const float* z, const float* dz, const float* B, const float* y, const float* e, int D_obs,
                              const float* L, int n_gen, long n_src, const int* idx, long n_idx_problems, int n_epochs,
                              int n_steps, int batch, long n_problems, int d, int order, int flags, const float* q_eff, int r,
                              int allow_constant, int n_params, float lr, float beta1, float beta2, float eps, float w_z,
                              float w_x, float w_reg, float w_sym, int l1, float threshold, int st_freq, int epoch0,
                              float near_band, float* params, float* m, float* v, int* step, float* mask, float* xi_out,
                              float* log, void* stream);

/* The three entries above WITHOUT an index table: the launch computes the row of every batch slot from an order seed, so
 * nothing runs between two launches of a fit and no index memory exists.  Each takes its sibling's arguments with
 * (idx, n_idx_problems, n_steps) replaced by
 *   order_seeds   (n_order_seeds) int64 ON THE DEVICE; n_order_seeds = 1: all problems walk the same order (as
 *                 n_idx_problems = 1), else n_order_seeds = n_problems
 *   shuffle       0: the loader with shuffle=False, see below
 * n_steps is implied: ceil(n_src / batch).  Batch slot b of step s in epoch e (global number epoch0 + e) is position
 * pos = s * batch + b of that epoch's order; its row is
 *   pos >= n_src                 -1, the canonical pad of the short last batch: not read, not counted
 *   shuffle == 0                 pos
 *   otherwise                    pi(pos), pi the permutation of [0, n_src) keyed by (order seed, epoch0 + e): an unbalanced
 *                                Feistel network over ceil(log2 n_src) bits, cycle-walked into [0, n_src); round keys from
 *                                the seed's 64-bit mix and the epoch number through the counter hash of
 *                                symode_seeded_subsamples (csrc/adam_order.hpp; device_adam.epoch_order is its numpy twin)
 * The order is a function of (order seed, global epoch, n_src) alone -- not of n_problems, batch, the launch cut or the
 * device -- so a fit cut into launches (epoch0 carried) agrees bit for bit with the fit in one launch, and each keyed entry
 * leaves bit for bit what its sibling leaves on the table symode_adam_order_table writes for the same arguments.  It is an
 * equivalent draw of the loader's shuffle, not a replay of torch's generator.
 * Refused beyond the sibling's checks: order_seeds == NULL (SYMODE_E_NULLPTR), n_order_seeds not in {1, n_problems},
 * n_src < 1 or n_src >= 2^31, batch < 1 (SYMODE_E_BADSIZE).  n_epochs == 0 or n_problems == 0: nothing to do.
 * replaces: train.py:491-547 (as the siblings) plus the per-epoch shuffle of DataLoader(train_dataset, batch_size,
 * shuffle=True) (main.py:36-38) that the table entries leave to the caller. */
int symode_adam_epochs_keyed(const float* x, const float* dx, long n_src, const long long* order_seeds, long n_order_seeds,
                             int shuffle, int n_epochs, int batch, long n_problems, int d, int order, int flags,
                             const float* q_eff, int r, int allow_constant, int n_params, float lr, float beta1, float beta2,
                             float eps, float w_x, float w_reg, int l1, float threshold, int st_freq, int epoch0,
                             float near_band, float* params, float* m, float* v, int* step, float* mask, float* xi_out,
                             float* log, void* stream);
int symode_adam_epochs_reversed_keyed(const float* x, const float* dx, const float* gx, const float* jgx, int n_g, long n_src,
                                      const long long* order_seeds, long n_order_seeds, int shuffle, int n_epochs, int batch,
                                      long n_problems, int d, int order, int flags, const float* q_eff, int r,
                                      int allow_constant, int n_params, float lr, float beta1, float beta2, float eps,
                                      float w_x, float w_reg, float w_sym, int l1, float threshold, int st_freq, int epoch0,
                                      float near_band, float* params, float* m, float* v, int* step, float* mask,
                                      float* xi_out, float* log, void* stream);
int symode_adam_epochs_latent_keyed(const float* z, const float* dz, const float* B, const float* y, const float* e, int D_obs,
                                    const float* L, int n_gen, long n_src, const long long* order_seeds, long n_order_seeds,
                                    int shuffle, int n_epochs, int batch, long n_problems, int d, int order, int flags,
                                    const float* q_eff, int r, int allow_constant, int n_params, float lr, float beta1,
                                    float beta2, float eps, float w_z, float w_x, float w_reg, float w_sym, int l1,
                                    float threshold, int st_freq, int epoch0, float near_band, float* params, float* m,
                                    float* v, int* step, float* mask, float* xi_out, float* log, void* stream);

/* The table the keyed entries walk, written out through the same device function: idx_out (n_epochs, n_order_seeds,
 * n_steps = ceil(n_src / batch), batch) int32, entry [e, s, step, b] the row of position step * batch + b in epoch
 * epoch0 + e under order_seeds[s] (device int64), -1 beyond n_src.  It is what idx of the table entries would have to hold
 * for the same fit: which rows a step saw, and the handle by which device and twin are compared.
 * Refused: order_seeds or idx_out NULL (SYMODE_E_NULLPTR); n_src < 1, n_src >= 2^31, batch < 1, n_order_seeds < 1,
 * n_epochs < 0, epoch0 < 0 (SYMODE_E_BADSIZE).  n_epochs == 0: nothing to do. */
int symode_adam_order_table(long n_src, int batch, const long long* order_seeds, long n_order_seeds, int shuffle, int epoch0,
                            int n_epochs, int* idx_out, void* stream);

/* The six epoch entries above as ONE descriptor entry, and with it a hyper-parameter grid in one launch: every problem may
 * have its own learning rate, L1 weight, threshold and regulariser weight.  `kind` names the loss (SYMODE_ADAM_*), exactly
 * one of idx / order_seeds non-NULL names the order: the table of symode_adam_epochs (idx, n_idx_problems, n_steps) or the
 * computed order of symode_adam_epochs_keyed (order_seeds, n_order_seeds, shuffle; n_steps is not read).  Every field has
 * the meaning of the argument of the same name in those entries; under SYMODE_ADAM_LATENT x, dx are z, dz, w_x is the weight
 * of mse_z (the latent entries' w_z) and w_obs the weight of mse_x (their w_x).  Pointers and counts that belong to another
 * kind are never read.
 *   hyper   NULL: the scalars lr, w_reg, threshold, w_sym apply and the entry leaves, bit for bit, what the entry of that
 *           kind and order leaves.
 *           else (n_problems, SYMODE_ADAM_HYPER = 4) fp32 row-major on the device, row s = [lr, w_reg, threshold, w_sym] of
 *           problem s; the four scalar fields are not read.  Workgroup s reads its row once, before its first step, and
 *           uses it wherever the scalar stands otherwise: the step size, the L1 term of the gradient, the thresholding
 *           event and its near count, the weight of the regulariser's gradient w_sym / w_x (REVERSED, LATENT: formed on
 *           the device as one fp32 division, 0 without a group element / generator) and w_sym in the value LATENT's
 *           freezing rule tests.  PLAIN does not read column 3.  Problem s of the launch leaves, bit for bit, what the
 *           scalar entry leaves for that problem alone with row s's four values.
 *           beta1, beta2, eps, w_x, w_obs, l1, st_freq and near_band are launch-wide.
 * Refused beyond the checks of the entry the descriptor names: J == NULL (SYMODE_E_NULLPTR); kind not one of the three,
 * idx and order_seeds both NULL or both given (SYMODE_E_BADSIZE; checked before everything else, the nothing-to-do cases
 * included); hyper not 4-byte aligned (SYMODE_E_ALIGN).
 * replaces: train.py:491-547 (as symode_adam_epochs and its siblings), per hyper-parameter point: one process
 * `python main.py --lr_sindy .. --w_sindy_reg .. --threshold .. --w_sym_reg ..` per candidate value. */
#define SYMODE_ADAM_PLAIN 0    /* symode_adam_epochs / _keyed */
#define SYMODE_ADAM_REVERSED 1 /* symode_adam_epochs_reversed / _reversed_keyed: gx, jgx, n_g, w_sym */
#define SYMODE_ADAM_LATENT 2   /* symode_adam_epochs_latent / _latent_keyed: lat_B, lat_y, lat_e, lat_L, D_obs, n_gen, w_obs, w_sym */
#define SYMODE_ADAM_HYPER 4    /* columns of hyper: lr, w_reg, threshold, w_sym */
typedef struct symode_adam_job {
    int kind;                  /* SYMODE_ADAM_* */
    /* data, read only, shared by all problems */
    const float* x;            /* (n_src, d); LATENT: z */
    const float* dx;           /* (n_src, d); LATENT: dz */
    long n_src;
    const float* gx;           /* REVERSED: (n_g, n_src, d) */
    const float* jgx;          /* REVERSED: (n_g, n_src, d, d) */
    int n_g;
    int D_obs;                 /* LATENT */
    const float* lat_B;        /* LATENT: (n_src, d, d) */
    const float* lat_y;        /* LATENT: (n_src, d) */
    const float* lat_e;        /* LATENT: (n_src), or NULL with D_obs == d */
    const float* lat_L;        /* LATENT: (n_gen, d, d), or NULL with n_gen == 0 */
    int n_gen;
    /* the order of the rows: the table ... */
    int n_steps;
    const int* idx;            /* (n_epochs, n_idx_problems, n_steps, batch) int32, or NULL */
    long n_idx_problems;       /* 1 or n_problems */
    /* ... or the order seeds */
    const long long* order_seeds; /* (n_order_seeds) int64 on the device, or NULL */
    long n_order_seeds;        /* 1 or n_problems */
    int shuffle;
    /* sizes and the coefficient map */
    int n_epochs, batch;
    long n_problems;
    int d, order, flags;
    const float* q_eff;        /* (d p, r), or NULL (the parameters are Xi) */
    int r, allow_constant, n_params;
    /* scalars; lr, w_reg, threshold and w_sym are not read when hyper is given */
    float lr, beta1, beta2, eps;
    float w_x;                 /* weight of the term with a gradient: mse, under LATENT mse_z */
    float w_obs;               /* LATENT: weight of mse_x */
    float w_reg, w_sym;
    int l1;
    float threshold;
    int st_freq, epoch0;
    float near_band;
    /* state (read and written back), Xi after the launch, the epoch records */
    float* params;             /* (n_problems, n_params) */
    float* m;
    float* v;
    int* step;                 /* (n_problems) */
    float* mask;               /* (n_problems, d p) */
    float* xi_out;             /* (n_problems, d p) */
    float* log;                /* (n_epochs, n_problems, 8; LATENT: SYMODE_ADAM_LOG_LATENT) */
    const float* hyper;        /* (n_problems, SYMODE_ADAM_HYPER), or NULL */
} symode_adam_job;
int symode_adam_run(const symode_adam_job* J, void* stream);

/* HOST function (no GPU work): least squares on the normal equations G = A^T A (n, n), C = A^T b (n, k), fp64
 * row-major host arrays; A had m_rows rows.  driver 0 = LAPACK gelsy semantics (pivoted QR rank rule with
 * rcond < 0 -> torch's default eps_fp32 * max(m_rows, n), minimum-norm solution), driver 1 = gels (full rank).
 * W (n, k) receives the solution, *rank_out the numerical rank.
 * replaces: torch.linalg.lstsq(A, B) on the ridge-augmented / block-diagonal system, sindy.py:288. */
int symode_host_lstsq_normal(const double* G, const double* C, int n, int k, long m_rows, int driver, double rcond,
                             double* W, int* rank_out);

/* HOST function (no GPU work): sequential-threshold least squares to convergence for S problems from their augmented Gram
 * matrices G (S, p+d, p+d) fp64 (symode_aug_gram / _gather output copied to the host); n_points rows each, ridge weight
 * gamma, strict > threshold on fp32-rounded coefficients, at most max_iter passes, driver as symode_host_lstsq_normal.
 * xi_out (S, d, p) fp32, mask_out (S, d, p) bytes, passes_out (S); near_out (S, may be NULL): coefficients met within
 * near_band of the threshold; fallback_out (S, may be NULL): singular systems handed to the
 * rank-revealing solve.
 * replaces: the per-seed loop of train.py:872-887 over solve_SINDy_one_step (sindy.py:250-315), unconstrained case. */
int symode_host_stlsq_sweep(const double* G, int S, int d, int p, long n_points, double gamma, double threshold, int max_iter,
                            int driver, double near_band, float* xi_out, unsigned char* mask_out, int* passes_out,
                            int* near_out, int* fallback_out);

/* Sequential-threshold least squares to convergence ON THE DEVICE, all problems in one launch (all pointers device memory):
 * what symode_host_stlsq_sweep does with driver = 1 (gels), restated -- ridge system Gtt + gamma^2 I on the current support,
 * per equation row (the host's joint block-diagonal system never mixes its blocks, so the eliminations and their order are
 * the same), pivoted Cholesky (largest remaining diagonal first, the first of equals), forward and back substitution, fp32
 * rounding, strict > (float)threshold on the still-active entries, until the problem's (d, p) mask repeats or max_iter
 * passes have run.  aug_gram (n_sets, p+d, p+d) fp64 as symode_aug_gram / _gather leave it; problem s reads set s % n_sets
 * (symode_trainer_grid's convention) and, with hyper (n_problems, 2) fp32 [gamma, threshold], row s in place of the two
 * scalars -- a hyper-parameter grid on shared matrices: no further data pass, no further collective.  hyper == NULL:
 * n_problems == n_sets and the scalars hold for all.  p <= 64, d <= 4.
 * xi_out (n_problems, d, p) fp32, mask_out (n_problems, d, p) bytes, passes_out, near_out (coefficients of an active entry
 * met within near_band of the threshold, summed over the passes), fell_out (n_problems) ints as the host defines them,
 * except: a pivot that is not > 0 sets fell_out[s] = 1 and ENDS problem s (its other outputs are then unspecified) -- the
 * caller solves those problems with symode_host_stlsq_sweep; the rank-revealing fallback and the gelsy rank rule are host
 * only.  n_points is accepted for symmetry with the host entry (only the gelsy rule reads it).
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, max_iter < 1, n_sets < 1, n_problems < n_sets or >= 2^31,
 * hyper == NULL with n_problems != n_sets (SYMODE_E_BADSIZE); any pointer but hyper NULL (SYMODE_E_NULLPTR); aug_gram not
 * 8-byte, hyper or an fp32 / int output not 4-byte aligned (SYMODE_E_ALIGN).
 * replaces: train.py:872-887 over sindy.py:250-315, unconstrained case. */
int symode_stlsq_sweep(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points, const float* hyper,
                       double gamma, double threshold, int max_iter, double near_band, float* xi_out, unsigned char* mask_out,
                       int* passes_out, int* near_out, int* fell_out, void* stream);

/* symode_stlsq_sweep under the equivariance constraint Xi = Q beta (+ const), EquivSINDy-c: the same loop, but per pass ONE
 * joint system over all equation rows in the r' = r + (allow_constant ? d : 0) free parameters.  aug_gram, n_sets, n_problems,
 * hyper, gamma, threshold, max_iter, near_band, n_points, mask_out, passes_out and near_out are symode_stlsq_sweep's.
 * q_solve (d p, r') fp64: row j p + k is equation j, library column k of Q (the reference's equation-major indexing of
 * Q[mask.flatten()], also when use_kron_product is false), then, with allow_constant, d unit columns, column r + j with its 1
 * in row j p.  q_xi (d p, r) fp32: the map that forms Xi, rows in Xi's (d, p) row-major order (it differs from q_solve's
 * first r columns exactly when use_kron_product is false).  Both are shared by all problems.
 * Per pass on the mask M (d, p): the columns of q_solve with a non-zero entry in a row of M, in ascending order (Qe, n of
 * them); Gq = Qe^T Gm Qe, cq = Qe^T cm in fp64 with Gm = blockdiag(Gtt + gamma^2 I)[M, M], cm = Gty[M] -- sums in ascending
 * (j, k, l), the upper triangle mirrored; pivoted Cholesky and substitutions as symode_stlsq_sweep; beta32 = (float) of the
 * solution in its r' slots, 0 in the others; Xi[j, k] = sum_c q_xi[j p + k, c] beta32[c] in fp32, c ascending,
 * + const32[j] at k = 0 with allow_constant; strict > (float)threshold on the still-active entries.
 * A pivot that is not > pivot_floor * (first pivot) sets fell_out[s] = 1 and ENDS problem s (its other outputs are then
 * unspecified): "possibly rank deficient" -- thresholding under the constraint routinely leaves collinear columns, whose last
 * pivot is round-off of either sign -- and the caller solves those problems on the host with the rank-revealing rule.
 * xi_out (n_problems, d, p) fp32: Xi of the last solve, unmasked; var_out (n_problems, r') fp32: [beta | const] of it.
 * p <= 64, d <= 4, r' <= 64.
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, r < 1, r' > 64, r' > d p, max_iter < 1, n_sets < 1, n_problems <
 * n_sets or >= 2^31, hyper == NULL with n_problems != n_sets, pivot_floor < 0 or not finite (SYMODE_E_BADSIZE); any pointer but
 * hyper NULL (SYMODE_E_NULLPTR); aug_gram or q_solve not 8-byte, q_xi, hyper or an fp32 / int output not 4-byte aligned
 * (SYMODE_E_ALIGN).
 * replaces: train.py:872-887 over sindy.py:250-315, constrained branch (regressor.constraint). */
int symode_stlsq_sweep_constrained(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points,
                                   const double* q_solve, const float* q_xi, int r, int allow_constant, const float* hyper,
                                   double gamma, double threshold, int max_iter, double near_band, double pivot_floor,
                                   float* xi_out, float* var_out, unsigned char* mask_out, int* passes_out, int* near_out,
                                   int* fell_out, void* stream);

/* symode_stlsq_sweep_constrained in its rank-revealing mode: every argument it shares with that entry means what it means
 * there, and a pass builds the same Gq, cq (same order of sums, exactly symmetric).  The solve of a pass is
 * symode_host_lstsq_normal's driver 0 with the rcond given here -- what the caller's host replay of a flagged problem performs
 * on every pass (lstsq_normal(Gq, cq, m, 'gelsy', SINGULAR_RCOND)) -- so problems whose support leaves Q's columns collinear
 * finish inside the one launch:
 *   the pivoted Cholesky with the fused forward substitution WITHOUT a pivot floor: a pivot that is not > 0 ends the
 *   factorisation, the remaining rows of R are zero (csrc/host_lstsq.cpp:55);
 *   the rank by xGELSY's loop over xLAIC1 estimates (csrc/host_lstsq.cpp:67-84, csrc/laic1.hpp -- one statement of xLAIC1 for
 *   host and device): position `rank` of the pivot order is accepted while smaxpr * rcond <= sminpr; rcond is the cut on the
 *   TRIANGULAR factor (the sweep passes lstsq.SINGULAR_RCOND = 1e-7);
 *   rank == n: the back substitution of symode_stlsq_sweep_constrained, identical arithmetic; rank == 0: the zero solution;
 *   0 < rank < n: the minimum-norm solution Y = Wm^T (Wm Wm^T)^-1 q, Wm = R[:rank, :], q the first `rank` entries of the forward
 *   substitution, in the host's order of operations (csrc/host_lstsq.cpp:102-132).
 * trunc_out (n_problems) ints: the passes of problem s solved with rank < n; rank_out (n_problems) ints: the rank of its last
 * pass's system (0 on an empty support).  fell_out[s] = 1 only when a diagonal of Wm Wm^T's Cholesky factor is not > 0; the
 * problem ENDS there (its other outputs are then unspecified) and stays the host's.
 * Refused before any GPU work: everything symode_stlsq_sweep_constrained refuses, with rcond in place of pivot_floor: rcond not
 * finite or outside (0, 1) (SYMODE_E_BADSIZE); trunc_out or rank_out NULL (SYMODE_E_NULLPTR) or not 4-byte aligned
 * (SYMODE_E_ALIGN).
 * replaces: train.py:872-887 over sindy.py:250-315, constrained branch (regressor.constraint), with torch.linalg.lstsq's
 * rank-revealing answer where the full-rank driver meets a singular system. */
int symode_stlsq_sweep_minnorm(const double* aug_gram, long n_sets, long n_problems, int d, int p, long n_points,
                               const double* q_solve, const float* q_xi, int r, int allow_constant, const float* hyper,
                               double gamma, double threshold, int max_iter, double near_band, double rcond, float* xi_out,
                               float* var_out, unsigned char* mask_out, int* passes_out, int* near_out, int* fell_out,
                               int* trunc_out, int* rank_out, void* stream);

/* symode_stlsq_sweep with the reversed symmetry regulariser, EquivSINDy-r: the same threshold loop, but per pass the
 * minimiser of mse + w_sym * reg on the support M, which is ONE joint linear system over all equation rows because the
 * regulariser's matrix couples them.  aug_gram, n_sets, n_problems, gamma, threshold, max_iter, near_band, n_points,
 * mask_out, passes_out and near_out are symode_stlsq_sweep's.  rev_gram (n_sets, d p, d p) fp64 as
 * symode_symreg_reversed_gram / _gather leave it: raw sums, rows and columns in Xi's (d, p) row-major order; problem s
 * reads set s % n_sets of both.  hyper NULL, or (n_problems, 3) fp32 [gamma, threshold, w_sym], row s in place of the three
 * scalars.  The launch takes the three values in fp32 with or without a table, so problem (g, k) of a grid is bit for bit
 * seed k of the scalar launch with point g's values.
 * Per pass: the support in ascending (j, k), n entries (n = 0: the zero solution, which ends the problem);
 * A[a, b] = [j_a == j_b] (Gtt[k_a, k_b] + gamma^2 [k_a == k_b]) + w_sym R[j_a p + k_a, j_b p + k_b] in fp64, the upper triangle
 * mirrored, b[a] = Gty[k_a, j_a] (the 1 / (N d) of mse and reg cancels); pivoted Cholesky and substitutions as
 * symode_stlsq_sweep_constrained (one statement, csrc/stlsq_joint.hpp): a pivot that is not > pivot_floor * (first pivot)
 * sets fell_out[s] = 1 and ENDS problem s (its other outputs are then unspecified), the caller solves it on the host;
 * Xi = (float) of the solution scattered into (d, p), zeros off the support; strict > (float)threshold on the still-active
 * entries.  xi_out (n_problems, d, p) fp32: the last solve.  d <= 4, p <= 64, d p <= 64.
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, d p > 64, max_iter < 1, n_sets < 1, n_problems < n_sets or >= 2^31,
 * hyper == NULL with n_problems != n_sets, gamma, threshold, w_sym or pivot_floor < 0 or not finite (SYMODE_E_BADSIZE); any
 * pointer but hyper NULL (SYMODE_E_NULLPTR); aug_gram or rev_gram not 8-byte, hyper or an fp32 / int output not 4-byte aligned
 * (SYMODE_E_ALIGN).
 * replaces: nothing in the reference; the stationarity condition of train.py:663-679 (sym_reg_type 'r') on the data of
 * train.py:626-629, thresholded as train.py:872-887. */
int symode_stlsq_sweep_symreg(const double* aug_gram, const double* rev_gram, long n_sets, long n_problems, int d, int p,
                              long n_points, const float* hyper, double gamma, double threshold, double w_sym, int max_iter,
                              double near_band, double pivot_floor, float* xi_out, unsigned char* mask_out, int* passes_out,
                              int* near_out, int* fell_out, void* stream);

/* The sparsity path of the least-squares fit ON THE DEVICE, all problems in one launch (all pointers device memory): stepwise
 * sparse regression by backward elimination, scored on held-out data -- no threshold is asked for.  aug_gram (n_sets, p+d,
 * p+d) and val_gram (n_val_sets, p+d, p+d) fp64 as symode_aug_gram / _gather leave them (raw sums; the second from the
 * held-out rows); problem s reads training set s % n_sets and validation set s % n_val_sets.  gamma = sqrt(w_sindy_reg) is the
 * ridge weight.  p <= 64, d <= 4.  Per equation row j, step t = 0 .. p has t columns removed:
 *   solve      t < p: (Gtt[M, M] + gamma^2 I) x = Gty[M, j] on the active columns M with the statements of one pass of
 *              symode_stlsq_sweep (pivoted Cholesky, fused forward substitution, back substitution, nothing contracted);
 *              v = (float)x on M and 0 elsewhere; t = p: v = 0.  path_xi[s, j, t, :] = v;
 *   errors     for H = the training and the validation matrix, in fp64 with w = (double)v: q_k = sum over l in M ascending of
 *              H[k][l] w_l from 0.0, r_k = w_k (q_k - 2 H[k][p+j]), e = H[p+j][p+j] then e += r_k for k ascending over M;
 *              rss_train[s, j, t], rss_val[s, j, t] = e.  The ridge term is in neither; nothing is clamped;
 *   eliminate  t < p: the active column with the smallest |v| (fp32 compare, the lowest index of equals) leaves,
 *              order[s, j, t] = that column; with two or more active columns the step counts in near_out[s] when the
 *              runner-up's |v| minus the smallest, both widened to fp64, is < near_band.
 * Then e_min = min_t rss_val[s, j, t], cut = (1 + tol) max(e_min, 0) + floor_rel val_gram[p+j][p+j], best[s, j] = the LARGEST
 * t with rss_val[s, j, t] <= cut (the argmin qualifies), xi_out[s, j, :] = path_xi[s, j, best, :] and mask_out its support.
 * A pivot that is not > 0 sets fell_out[s] = 1 and ENDS problem s (its other outputs are then unspecified), as for
 * symode_stlsq_sweep.  n_points is accepted for symmetry with the siblings.
 * path_xi (n_problems, d, p+1, p) fp32; order (n_problems, d, p) ints; rss_train, rss_val (n_problems, d, p+1) fp64; best
 * (n_problems, d) ints; xi_out (n_problems, d, p) fp32; mask_out (n_problems, d, p) bytes; near_out, fell_out (n_problems) ints.
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, n_sets < 1, n_problems < n_sets or >= 2^31, n_val_sets < 1 or
 * > n_problems, gamma, tol, floor_rel or near_band < 0 or not finite (SYMODE_E_BADSIZE); any pointer NULL (SYMODE_E_NULLPTR);
 * aug_gram, val_gram, rss_train or rss_val not 8-byte, an fp32 / int output not 4-byte aligned (SYMODE_E_ALIGN).
 * Added to ABI version 8 (nothing existing changed).
 * replaces: nothing in the reference; the threshold loop of train.py:872-887 with the threshold chosen by held-out error. */
int symode_stlsq_path(const double* aug_gram, const double* val_gram, long n_sets, long n_val_sets, long n_problems, int d, int p,
                      long n_points, double gamma, double tol, double floor_rel, double near_band, float* path_xi, int* order,
                      double* rss_train, double* rss_val, int* best, float* xi_out, unsigned char* mask_out, int* near_out,
                      int* fell_out, void* stream);

/* symode_stlsq_path with the reversed symmetry regulariser, EquivSINDy-r: the sparsity path of the minimiser of
 * mse + w_sym * reg, so that the regularised fit no longer asks for a threshold either.  The regulariser's matrix couples the
 * equation rows, so the path is ONE chain over the joint (d, p) support of n0 = d p <= 64 entries, not one per row.
 * aug_gram, val_gram, n_sets, n_val_sets, n_problems, n_points, tol, floor_rel and near_band are symode_stlsq_path's; rev_gram
 * (n_sets, d p, d p) fp64, pivot_floor and the fp32 rounding of gamma and w_sym are symode_stlsq_sweep_symreg's.  hyper NULL,
 * or (n_problems, 2) fp32 [gamma, w_sym], row s in place of the two scalars; the launch takes the two values in fp32 with or
 * without a table, so problem (g, k) of a table is bit for bit the scalar launch on set k with row g's values.
 * Step t = 0 .. n0 has t entries of the support M removed:
 *   solve      t < n0: the statements of one pass of symode_stlsq_sweep_symreg on M (support in ascending (j, k), its A and b,
 *              csrc/stlsq_joint.hpp) -- step 0 is bit for bit that entry with max_iter = 1, threshold = 0; a pivot that is
 *              not > pivot_floor * (first pivot), or not > 0, sets fell_out[s] = 1 and ENDS problem s (its other outputs are
 *              then unspecified), the caller solves it on the host; v = (float) of the solution scattered to (d, p), zeros
 *              off M; t = n0: v = 0.  path_xi[s, t, :, :] = v;
 *   scores     in fp64 with w = (double)v, nothing contracted, nothing clamped.  For H = the training and the validation
 *              matrix: per row j, with M_j the row's columns, q_k = sum over l in M_j ascending of H[k][l] w_jl from 0.0,
 *              r_k = w_jk (q_k - 2 H[k][p+j]), e_j = H[p+j][p+j] then e_j += r_k for k ascending over M_j (symode_stlsq_path's
 *              form); the score starts at 0.0 and takes e_j for j ascending: mse_train[s, t], mse_val[s, t] (raw sums, the
 *              ridge term in neither).  reg_train[s, t] = v^T R v over the flat index b = j p + k: q_b = sum over a in M
 *              ascending of R[b][a] w_a from 0.0, r_b = w_b q_b, the form from 0.0 takes r_b for b ascending over M.  The
 *              regulariser is not scored on held-out data;
 *   eliminate  t < n0: the active entry with the smallest |v| (fp32 compare, the lowest flat index j p + k of equals) leaves,
 *              order[s, t] = that flat index; with two or more active entries the step counts in near_out[s] when the
 *              runner-up's |v| minus the smallest, both widened to fp64, is < near_band.
 * Then Vyy = sum_j val_gram[p+j][p+j] (from 0.0, j ascending: the empty model's mse_val), e_min = min_t mse_val[s, t],
 * cut = (1 + tol) max(e_min, 0) + floor_rel Vyy, best[s] = the LARGEST t with mse_val[s, t] <= cut, xi_out[s] =
 * path_xi[s, best] (solved once more: the same bits) and mask_out[s] its support, the entries order[s, best:].
 * path_xi (n_problems, n0+1, d, p) fp32; order (n_problems, n0) ints; mse_train, reg_train, mse_val (n_problems, n0+1) fp64;
 * best, near_out, fell_out (n_problems) ints; xi_out (n_problems, d, p) fp32; mask_out (n_problems, d, p) bytes.
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, d p > 64, n_sets < 1, n_problems < n_sets or >= 2^31, n_val_sets < 1
 * or > n_problems, gamma, w_sym, tol, floor_rel, near_band or pivot_floor < 0 or not finite (SYMODE_E_BADSIZE); any pointer
 * but hyper NULL (SYMODE_E_NULLPTR); aug_gram, rev_gram, val_gram or a score array not 8-byte, hyper or an fp32 / int output
 * not 4-byte aligned (SYMODE_E_ALIGN).
 * Added to ABI version 8 (nothing existing changed).
 * replaces: nothing in the reference; the threshold loop of train.py:872-887 on the stationarity condition of
 * train.py:663-679 (sym_reg_type 'r'), with the threshold chosen by held-out error. */
int symode_stlsq_path_symreg(const double* aug_gram, const double* rev_gram, const double* val_gram, long n_sets, long n_val_sets,
                             long n_problems, int d, int p, long n_points, const float* hyper, double gamma, double w_sym,
                             double tol, double floor_rel, double near_band, double pivot_floor, float* path_xi, int* order,
                             double* mse_train, double* reg_train, double* mse_val, int* best, float* xi_out,
                             unsigned char* mask_out, int* near_out, int* fell_out, void* stream);

/* Block-bootstrap replicas of Gram matrices ON THE DEVICE, one launch (all pointers device memory).  A Gram matrix is a sum over
 * rows, so a bootstrap replica that resamples whole chunks of a seed's rows is an integer-weighted sum of the chunks' matrices.
 * chunk (n_seeds, n_chunks, n, n) fp64; seeds (n_seeds) 64-bit integers; out (n_seeds * n_replicas, n, n) fp64, replica b of seed
 * k at index k * n_replicas + b; counts_out NULL or (n_seeds * n_replicas, n_chunks) ints.  With C = n_chunks:
 *   draw   w = seed_words(seed_words(seeds[k]) + b) modulo 2^64 and, for t = 0 .. C-1, u = subsample_key(low32(w), high32(w), t)
 *          (the two counter hashes of symode_seeded_subsamples, csrc/adam_order.hpp); draw t lands on chunk (u * C) >> 32 in
 *          64-bit arithmetic, which is < C; count[c] = the draws that landed on c, so every row of counts sums to C;
 *   sum    out[e] = 0.0, then out[e] = out[e] + (double)count[c] * chunk[k, c, e] for c ascending, chunks with count 0 skipped,
 *          one multiply and one add per term, nothing contracted; each of the n^2 entries by itself, so a symmetric input gives
 *          a symmetric output, and a replica does not depend on the seeds or the replica count it is launched with.
 * n is generic: p + d for the augmented matrices, d p for the regulariser's.
 * Refused before any GPU work: n_chunks < 1 or > 1024, n < 1 or > 68, n_replicas < 1, n_seeds < 1, n_seeds * n_replicas >= 2^31
 * (what symode_stlsq_sweep refuses as a problem count) (SYMODE_E_BADSIZE); chunk, seeds or out NULL (SYMODE_E_NULLPTR); chunk,
 * seeds or out not 8-byte, counts_out not 4-byte aligned (SYMODE_E_ALIGN).
 * Added to ABI version 8 (nothing existing changed).
 * replaces: nothing in the reference (the block bootstrap of ensemble SINDy on Gram matrices). */
int symode_gram_resample(const double* chunk, const long long* seeds, long n_seeds, int n_chunks, int n, int n_replicas, double* out,
                         int* counts_out, void* stream);

/* Bagging of the device STLSQ fit: aggregate the replica fits of every seed and refit on the terms that survive often enough, all
 * problems in one launch (all pointers device memory).  aug_gram (n_seeds, p+d, p+d) fp64, each seed's OWN matrix; rep_xi
 * (n_seeds * n_replicas, d, p) fp32, rep_mask (same shape) bytes and rep_fell (n_seeds * n_replicas) ints are the xi_out, mask_out
 * and fell_out of symode_stlsq_sweep on the n_seeds * n_replicas matrices of symode_gram_resample.  Problem s works on seed
 * k = s % n_seeds at the inclusion level tau_table[s] (n_problems ints), or tau_milli for all when tau_table is NULL, in
 * thousandths, 0 .. 1000: a grid of levels is more problems on the same replica outputs.  p <= 64, d <= 4.
 *   statistics  over the seed's replicas b ascending, one with rep_fell set left out: valid = the replicas that remain; per term,
 *               count = the valid replicas whose mask keeps it and, over those, in fp64: sum from 0.0, mean = sum / count, ss =
 *               sum from 0.0 of (x - mean)^2 in a second pass, std = sqrt(ss / count); count == 0: mean = std = 0;
 *   inclusion   a term is kept iff valid > 0 and 1000 count >= tau valid (integers, exact);
 *   refit       per equation row, one pass of symode_stlsq_sweep's solve on the kept support from aug_gram[k] with ridge gamma,
 *               rounded to fp32; an empty row is zeros.  A pivot that is not > 0 sets fell_out[s] = 1 (the row is then zeros;
 *               the caller solves the problem on the host); nothing else is flagged.
 * xi_out (n_problems, d, p) fp32, mask_out (n_problems, d, p) bytes (the kept terms), fell_out (n_problems) ints; written by the
 * problems s < n_seeds only: count_out (n_seeds, d, p) ints, valid_out (n_seeds) ints, mean_out, std_out (n_seeds, d, p) fp64.
 * tau = 0 is bit for bit symode_stlsq_sweep with max_iter = 1 and threshold = 0 on the same matrix (while a replica is valid).
 * Refused before any GPU work: d < 1, d > 4, p < 1, p > 64, n_seeds < 1, n_problems < n_seeds, >= 2^31 or not a multiple of
 * n_seeds, n_replicas < 1, n_seeds * n_replicas >= 2^31, tau_table NULL with tau_milli outside 0 .. 1000 (the caller checks a
 * table before it uploads it), gamma < 0 or not finite (SYMODE_E_BADSIZE); any pointer but tau_table NULL (SYMODE_E_NULLPTR);
 * aug_gram, mean_out or std_out not 8-byte, tau_table or another fp32 / int array not 4-byte aligned (SYMODE_E_ALIGN).
 * Added to ABI version 8 (nothing existing changed).
 * replaces: nothing in the reference (aggregation and refit of ensemble SINDy). */
int symode_stlsq_bag(const double* aug_gram, long n_seeds, long n_problems, int d, int p, int n_replicas, const float* rep_xi,
                     const unsigned char* rep_mask, const int* rep_fell, const int* tau_table, int tau_milli, double gamma,
                     float* xi_out, unsigned char* mask_out, int* fell_out, int* count_out, int* valid_out, double* mean_out,
                     double* std_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYMODE_H */
