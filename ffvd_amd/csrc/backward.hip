// The multi-kernel backward pass behind a forward iteration (kernels: grad.hip): its workspace, the launch
// sequences of the explicit-U and the collapsed branch, and the gradients' way out.  Like the forward iteration in abi.hip, every
// argument block is built in ONE place that both branches share; a branch sets only what differs, behind the call.
#include "handle.h"
#include "kernels_f32.h"
#include "grad.h"

#include <cstring>

using namespace ffvd;

// the `if (cfg.grad)` part of create_impl: allocation order and sizes are part of ffvd_workspace_bytes and of h->allocs
int ffvd::alloc_grad_workspace(ffvd_handle *h) {
    const ffvd_config &c = h->cfg;
    ffvd_handle::GradWs &g = h->gw;
    const size_t Mp = h->Mp, Tp = h->Tp, Dl = h->Dl, P = h->P;
    const bool grad_a = c.branch == FFVD_BRANCH_A;
    const bool grad_ref = c.branch == FFVD_BRANCH_B && c.route == FFVD_ROUTE_REFERENCE;    // backward pass in the reference's op order
    const size_t nbt = h->nbatch, msq = Mp * Mp, nblk = Tp / 64, nblk2 = Mp / 64, S = c.S_local, J = c.Ydim;
    g.ngam = atb_ntiles_sym64(h->Mp);        // the Gamma launch uses the 64 x 64-tile kernel
    g.sp_stride = c.D * c.Ydim + 2 * c.Ydim + (int)Dl;
    HIP_TRY(dev_alloc(h, &g.Acopy, nbt * msq));      HIP_TRY(dev_alloc(h, &g.u, nbt * Mp));
    HIP_TRY(dev_alloc(h, &g.LAinv, nbt * msq));      HIP_TRY(dev_alloc(h, &g.Gamma, nbt * msq));
    HIP_TRY(dev_alloc(h, &g.gam_part, nbt * g.ngam)); HIP_TRY(dev_alloc(h, &g.uku, nbt));
    if (c.dtype == FFVD_F32C) HIP_TRY(dev_alloc(h, &g.Gam32, nbt * msq));                          // E formed on the fly from fp32 operands
    else if (P <= 6) HIP_TRY(dev_alloc(h, &g.rp, bwd_fused_rp_doubles((int)Mp, (int)Tp, (int)nbt)));   // fused E reductions
    else HIP_TRY(dev_alloc(h, &g.E, nbt * Tp * Mp));
    if (grad_ref && c.dtype != FFVD_F32C) HIP_TRY(dev_alloc(h, &g.fsq, nbt));
    HIP_TRY(dev_alloc(h, &g.rsum, nbt * Tp));        HIP_TRY(dev_alloc(h, &g.ez, nbt * Tp * P));
    HIP_TRY(dev_alloc(h, &g.kfu, nbt * Tp));
    HIP_TRY(dev_alloc(h, &g.cs_part, nbt * nblk * Mp)); HIP_TRY(dev_alloc(h, &g.etx_part, nbt * nblk * Mp * P));
    HIP_TRY(dev_alloc(h, &g.rx2_part, nbt * nblk * P));
    HIP_TRY(dev_alloc(h, &g.dz_unit, nbt * c.M * P)); HIP_TRY(dev_alloc(h, &g.dll_unit, nbt * P));
    HIP_TRY(dev_alloc(h, &g.dls_unit, nbt));
    HIP_TRY(dev_alloc(h, &g.Asum, Dl * msq));  HIP_TRY(dev_alloc(h, &g.GamSum, Dl * msq)); HIP_TRY(dev_alloc(h, &g.Gs, Dl * msq));
    HIP_TRY(dev_alloc(h, &g.gsum, Dl * msq));  HIP_TRY(dev_alloc(h, &g.P1, Dl * msq));     HIP_TRY(dev_alloc(h, &g.KGK, Dl * msq));
    HIP_TRY(dev_alloc(h, &g.Epsi, Dl * msq));
    // (the reference route factorises H = I + F^T F / Q itself: its backward pass is the whitened one by construction)
    g.whitened = c.branch == FFVD_BRANCH_B && (!h->sw.grad_explicit || grad_ref);
    if (g.whitened) {
        HIP_TRY(dev_alloc(h, &g.T1, nbt * msq));
        HIP_TRY(dev_alloc(h, &g.wv, nbt * Mp));    HIP_TRY(dev_alloc(h, &g.bw, nbt * Mp));
        HIP_TRY(dev_alloc(h, &g.Ident, msq));      HIP_TRY(dev_alloc(h, &g.P2, Dl * msq)); HIP_TRY(dev_alloc(h, &g.P3, Dl * msq));
        launch_set_identity(h->stream, g.Ident, 0, 0, (int)Mp, 1);
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(dev_alloc(h, &g.rsum2, Dl * Mp));  HIP_TRY(dev_alloc(h, &g.ez2, Dl * Mp * P));
    HIP_TRY(dev_alloc(h, &g.cs2, Dl * nblk2 * Mp)); HIP_TRY(dev_alloc(h, &g.etx2, Dl * nblk2 * Mp * P));
    HIP_TRY(dev_alloc(h, &g.rx22, Dl * nblk2 * P));
    HIP_TRY(dev_alloc(h, &g.dz_kuu, Dl * c.M * P)); HIP_TRY(dev_alloc(h, &g.dll_kuu, Dl * P)); HIP_TRY(dev_alloc(h, &g.dls_kuu, Dl));
    HIP_TRY(dev_alloc(h, &g.shared_part, S * g.sp_stride));
    {   // every parameter gradient lives in ONE block (see GradWs::pack); the six small shared-parameter gradients are
        // contiguous inside it: one fill per backward pass instead of six memsets
        auto seg = [](size_t n) { return (n + 31) / 32 * 32; };
        g.small_count = (size_t)c.D + (size_t)c.D * P + (size_t)c.D + (size_t)c.D * J + J + J * J;
        const size_t nZ = (size_t)c.M * P, nU = grad_a ? (size_t)c.M * c.D : 0, nX = S * (c.T + 1) * c.D;
        const size_t oZ = seg(8), oS = oZ + seg(nZ), oU = oS + seg(g.small_count), oX = oU + seg(nU);
        g.pack_shared = oX; g.pack_total = oX + seg(nX);
        HIP_TRY(dev_alloc(h, &g.pack, g.pack_total));
        HIP_TRY(hipMemsetAsync(g.pack, 0, g.pack_total * sizeof(double), h->stream));     // the padding stays zero
        g.dZ = g.pack + oZ; g.dlogvar = g.pack + oS; g.dX = g.pack + oX;
        if (grad_a) g.dU = g.pack + oU;
        g.dloglen = g.dlogvar + c.D; g.dlogQ = g.dloglen + (size_t)c.D * P; g.dCC = g.dlogQ + c.D;
        g.dDD = g.dCC + (size_t)c.D * J; g.dlogR = g.dDD + J;
    }
    if (!grad_a && c.kernel_kind != FFVD_KERNEL_SE) HIP_TRY(dev_alloc(h, &g.xsq, nbt));      // LinearK, collapsed branch: sum_t |x_t|^2 per unit
    if (grad_a) {
        HIP_TRY(dev_alloc(h, &g.Gu, nbt * (Mp + NB) * Mp));   HIP_TRY(dev_alloc(h, &g.Gsum, Dl * (Mp + NB) * Mp));
        HIP_TRY(dev_alloc(h, &g.r, nbt * Tp));                HIP_TRY(dev_alloc(h, &g.dalpha, nbt));
        HIP_TRY(dev_alloc(h, &g.xsq, nbt));
        HIP_TRY(dev_alloc(h, &g.ucol, Dl * Mp));              HIP_TRY(dev_alloc(h, &g.beta, Dl * Mp));
        HIP_TRY(dev_alloc(h, &g.du, Dl * Mp));                HIP_TRY(dev_alloc(h, &g.GammaA, Dl * msq));
        HIP_TRY(dev_alloc(h, &g.Lclean, Dl * msq));           // (g.dU: a segment of g.pack)
    }
    return FFVD_OK;
}

// ---- argument blocks of the backward pass's launches: each built once, shared by both branches -------------------------------------
// LinearK (kernels.py:270-281): K = (x s2) z^T has no Hadamard factor in its chain rule and its Kdiag_t = s2 |x_t|^2 depends on the
// inputs -- `kind`, `linear` and `no_hadamard` below, plus sum_t |x_t|^2 per unit (xsq_unit)

// reductions of the K_fu side's E (e_reduce, e_finish).  Behind the call: u_per_dim (explicit-U branch), the fp32 operands (fp32 path)
static EReduceArgs grad_efu_args(const ffvd_handle *h, const double *Kf, const double *u) {
    const ffvd_config &c = h->cfg; const ffvd_handle::GradWs &g = h->gw; const ffvd_params &p = h->cur;
    EReduceArgs er{};
    er.kind = c.kernel_kind; er.variance = h->variance;
    er.E = g.E; er.e_stride = (size_t)h->Tp * h->Mp; er.Kf = Kf; er.u = u; er.u_stride = h->Mp; er.x_is_z = 0;
    er.x = p.X; er.x_chain_stride = (size_t)(c.T + 1) * c.D; er.x_ld = c.D; er.x_cols = c.D; er.ctrl = h->ctrl; er.C = c.C;
    er.Z = p.Z; er.len = h->len; er.T = c.T; er.Tp = h->Tp; er.M = c.M; er.Mp = h->Mp; er.P = h->P; er.Dl = h->Dl; er.b0 = 0;
    er.nb = h->nbatch; er.nblk = h->Tp / 64; er.rsum = g.rsum; er.ez = g.ez; er.kfu = g.kfu; er.cs_part = g.cs_part;
    er.etx_part = g.etx_part; er.rx2_part = g.rx2_part;
    return er;
}

// latent trajectories (dx) and the per-chain partials of the shared parameters: the same block on both branches
static DxArgs grad_dx_args(const ffvd_handle *h, int S_total) {
    const ffvd_config &c = h->cfg; const ffvd_handle::GradWs &g = h->gw; const ffvd_params &p = h->cur;
    DxArgs dx{};
    dx.kind = c.kernel_kind; dx.variance = h->variance;
    dx.X = p.X; dx.Y = h->Y; dx.CC = p.CC; dx.DD = p.DD; dx.log_Rchols = p.log_Rchols; dx.log_Q = p.log_Q; dx.len = h->len;
    dx.rsum = g.rsum; dx.ez = g.ez; dx.kfu = g.kfu; dx.S = c.S_local; dx.S_total = S_total; dx.T = c.T; dx.Tp = h->Tp; dx.D = c.D;
    dx.P = h->P; dx.Ydim = c.Ydim; dx.Dl = h->Dl; dx.d_begin = c.d_begin; dx.shared_terms = c.shared_terms; dx.dX = g.dX;
    dx.T_norm = c.T_total; dx.skip_x0 = (c.T_total > 0 && c.t_begin > 0) ? 1 : 0;      // T-shards: the job's 1 / T, x_0 on the first shard
    return dx;
}

// grad_finalize.  Behind the call: branch_a, dalpha_unit, du_dim, U, dU (explicit-U branch); gam_part, ngam, trpart, ntr, hterms, uku
// (collapsed branch).  T_norm and replicated_skip are 0 on the explicit-U branch: ffvd_create rejects a T-shard (T_total > 0) there
static GradFinalArgs grad_final_args(const ffvd_handle *h, int S_total) {
    const ffvd_config &c = h->cfg; const ffvd_handle::GradWs &g = h->gw; const ffvd_params &p = h->cur;
    GradFinalArgs gf{};
    gf.T = c.T; gf.D = c.D; gf.P = h->P; gf.M = c.M; gf.Mp = h->Mp; gf.Ydim = c.Ydim; gf.Dl = h->Dl; gf.d_begin = c.d_begin;
    gf.S = c.S_local; gf.S_total = S_total; gf.shared_terms = c.shared_terms; gf.prior_type = c.prior_type;
    gf.T_norm = c.T_total; gf.replicated_skip = (c.T_total > 0 && c.t_begin > 0) ? 1 : 0;
    gf.Z = p.Z; gf.logvar = p.logvariance; gf.loglen = p.loglengthscales; gf.log_Q = p.log_Q; gf.CC = p.CC; gf.DD = p.DD;
    gf.log_Rchols = p.log_Rchols; gf.dz_unit = g.dz_unit; gf.dll_unit = g.dll_unit; gf.dls_unit = g.dls_unit;
    gf.dz_kuu = g.dz_kuu; gf.dll_kuu = g.dll_kuu; gf.dls_kuu = g.dls_kuu; gf.shared_part = g.shared_part;
    gf.sp_stride = g.sp_stride; gf.dZ = g.dZ; gf.dlogvar = g.dlogvar; gf.dloglen = g.dloglen; gf.dlogQ = g.dlogQ;
    gf.dCC = g.dCC; gf.dDD = g.dDD; gf.dlogR = g.dlogR;
    gf.kind = c.kernel_kind; gf.xsq_unit = g.xsq;
    return gf;
}

// K_uu side: E_psi (Mp x Mp per latent dim, its rows the inducing inputs themselves) reduced into the *_kuu arrays
static void enqueue_kuu_reduce(const ffvd_handle *h, hipStream_t stream) {
    const ffvd_config &c = h->cfg; const ffvd_handle::GradWs &g = h->gw;
    const int Mp = h->Mp;
    EReduceArgs ek{};
    ek.kind = c.kernel_kind; ek.variance = h->variance;
    ek.E = g.Epsi; ek.e_stride = (size_t)Mp * Mp; ek.Kf = nullptr; ek.u = nullptr; ek.x_is_z = 1; ek.Z = h->cur.Z; ek.len = h->len;
    ek.T = c.M; ek.Tp = Mp; ek.M = c.M; ek.Mp = Mp; ek.P = h->P; ek.Dl = h->Dl; ek.b0 = 0; ek.nb = h->Dl; ek.nblk = Mp / 64;
    ek.rsum = g.rsum2; ek.ez = g.ez2; ek.kfu = nullptr; ek.cs_part = g.cs2; ek.etx_part = g.etx2; ek.rx2_part = g.rx22;
    launch_e_reduce(stream, ek);
    launch_e_finish(stream, ek, g.dz_kuu, g.dll_kuu, g.dls_kuu);
}

// The K_fu side's E = (2 K_fu Gamma + alpha delta u^T) [o K_fu] and its reductions (into er's outputs; e_finish follows at the
// caller), one of three ways: fp32 contractions, fused, or materialise then reduce.  Each way's argument block is built here, its
// only place.  rvec != nullptr is the explicit-U branch: Gamma and u are per latent dim there and the residuals r stand in for delta
static void launch_e_product(const ffvd_handle *h, hipStream_t s, EReduceArgs &er, const double *Kf, const double *Gamma, const double *u,
                             const double *rvec) {
    const ffvd_config &c = h->cfg; const ffvd_handle::GradWs &g = h->gw; const ffvd_params &p = h->cur;
    const int Mp = h->Mp, Tp = h->Tp, nb = h->nbatch, lin = c.kernel_kind != FFVD_KERNEL_SE;
    const size_t msq = (size_t)Mp * Mp, fstride = (size_t)Tp * Mp;
    if (c.dtype == FFVD_F32C) {
        // fp32 contractions (BASELINE configs[3]; collapsed branch only): Gamma rounded once, R = K_fu Gamma on v_mfma_f32_32x32x2_f32 into
        // the buffer F occupied in the forward pass, then E_tm = (2 R_tm + alpha delta_t u_m) K_tm formed on the fly inside the
        // reduction kernel with every sum in fp64 (E itself is never stored)
        launch_to_f32(s, Gamma, g.Gam32, (size_t)nb * msq);
        ProjF32Args pg{};
        pg.Kf = h->Kf32; pg.kf_stride = fstride; pg.Bunit = g.Gam32; pg.bunit_stride = msq; pg.F = h->F32; pg.f_stride = fstride;
        pg.sqpart = nullptr; pg.Tp = Tp; pg.Mp = Mp; pg.Dl = h->Dl; pg.b0 = 0; pg.nb = nb;
        launch_proj_gemm_f32(s, pg);
        er.E = nullptr; er.Kf = nullptr; er.R32 = h->F32; er.Kf32 = h->Kf32; er.Xd = p.X; er.log_Q = p.log_Q; er.D = c.D;
        er.d_begin = c.d_begin;
        launch_e_reduce(s, er);
    } else if (g.rp) {
        // P <= 6: E formed and reduced tile by tile, it never reaches HBM
        BwdFusedArgs bf{};
        bf.Kf = Kf; bf.kf_stride = fstride; bf.Gamma = Gamma; bf.g_stride = msq; bf.u = u; bf.u_stride = Mp;
        bf.X = p.X; bf.ctrl = h->ctrl; bf.Z = p.Z; bf.log_Q = p.log_Q; bf.T = c.T; bf.Tp = Tp; bf.D = c.D; bf.C = c.C;
        bf.M = c.M; bf.Mp = Mp; bf.P = h->P; bf.Dl = h->Dl; bf.d_begin = c.d_begin; bf.b0 = 0; bf.nb = nb; bf.rp = g.rp;
        bf.cs_part = g.cs_part; bf.etx_part = g.etx_part; bf.rsum = g.rsum; bf.ez = g.ez; bf.kfu = g.kfu; bf.rx2_part = g.rx2_part;
        bf.linear = lin;
        if (rvec) { bf.per_dim = 1; bf.rvec = rvec; }
        launch_bwd_fused(s, bf);
    } else {
        // P > 6 (BASELINE config 5: P = 17): materialise E and reduce it in a second kernel
        AtbArgs ae{};
        ae.mode = ATB_BWD_E; ae.A = Kf; ae.a_stride = fstride; ae.lda = Mp; ae.nA = Tp; ae.a_rowmajor = 1;   // K_fu itself
        ae.B = Gamma; ae.b_stride = msq; ae.ldb = Mp; ae.nB = Mp; ae.rows = Mp;
        ae.C = g.E; ae.c_stride = fstride; ae.ldc = Mp; ae.nb = nb; ae.b0 = 0; ae.Dl = h->Dl; ae.d_begin = c.d_begin;
        ae.log_Q = p.log_Q; ae.u = u; ae.u_stride = Mp; ae.X = p.X; ae.T = c.T; ae.D = c.D;
        ae.Kf = Kf; ae.kf_stride = fstride; ae.ldkf = Mp; ae.no_hadamard = lin;
        if (rvec) { ae.b_per_dim = 1; ae.u_per_dim = 1; ae.rvec = rvec; }
        launch_atb(s, ae);
        launch_e_reduce(s, er);
    }
}

// C = A^T B per latent dim, all three Mp x Mp (ATB_PLAIN).  Both operands, both strides and krange (which k-tiles are read: grad.h)
// are set on every call: no product depends on what the one before it left behind
static AtbArgs mm_args(const ffvd_handle *h) {
    const int Mp = h->Mp;
    AtbArgs ap{};
    ap.mode = ATB_PLAIN; ap.lda = Mp; ap.nA = Mp; ap.ldb = Mp; ap.nB = Mp; ap.rows = Mp; ap.ldc = Mp; ap.nb = h->Dl; ap.Dl = h->Dl;
    ap.c_stride = (size_t)Mp * Mp;
    return ap;
}
static void mm(hipStream_t stream, AtbArgs ap, const double *A, size_t a_stride, const double *B, size_t b_stride, double *C, int krange = 0) {
    ap.A = A; ap.a_stride = a_stride; ap.B = B; ap.b_stride = b_stride; ap.C = C; ap.krange = krange;
    launch_atb(stream, ap);
}

// Backward pass of the explicit-U branch (closed form: oracle/ffvd_grad_oracle.py nll_grad_explicit_u).  The T x M work
// reuses the collapsed branch's kernels: one Gram pass (G = K_uf K_fu and g_r = K_uf r per unit) and the fused E
// product with Gamma := alpha K^-1 / 2, delta := r, u := beta = L^-T u; everything else is M x M per latent dim.
static int enqueue_grad_a(ffvd_handle *h, int S_total) {
    const ffvd_config &c = h->cfg;
    ffvd_handle::GradWs &g = h->gw;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl, nb = h->nbatch, S = c.S_local;
    const size_t msq = (size_t)Mp * Mp, kstride = 2 * msq, fstride = (size_t)Tp * Mp, gstride = (size_t)(Mp + NB) * Mp;
    hipStream_t s = h->stream;
    const ffvd_params &p = h->cur;
    const double *W = h->Kuu + msq;                                                     // L^-T rows, per dim stride kstride
    // beta = W u,  r = delta - mean,  dl/dalpha per unit
    launch_ucols(s, p.U, c.M, Mp, c.D, c.d_begin, Dl, g.ucol);
    launch_matvec(s, W, kstride, g.ucol, Mp, Mp, g.beta, 1, Mp, Mp, Dl);
    const int kind = c.kernel_kind;
    launch_resid_a(s, kind, p.X, h->ctrl, c.C, h->fmean, h->rowsq, h->variance, p.log_Q, c.T, Tp, c.D, Dl, c.d_begin,
                   h->ngr ? h->ngr : h->ng, nb, g.r, g.dalpha, g.xsq);
    // G = K_uf K_fu (lower tiles) and g_r = K_uf r (row Mp) per unit, then summed over the chains
    GramArgs gg{};
    gg.mode = GRAM_PLAIN; gg.A = h->F; gg.a_stride = fstride; gg.rows = Tp; gg.with_row = 1; gg.brow = Mp; gg.rvec = g.r;
    gg.X = p.X; gg.log_Q = p.log_Q; gg.T = c.T; gg.D = c.D; gg.Mp = Mp; gg.Dl = Dl; gg.d_begin = c.d_begin; gg.b0 = 0; gg.nb = nb;
    gg.yn_over_batch = 1.0; gg.H = g.Gu; gg.h_stride = gstride;
    launch_gram(s, gg);
    launch_chain_sum(s, g.Gu, gstride, S, Dl, (size_t)(Mp + 1) * Mp, g.Gsum, gstride);
    // M x M chain per dim:  dW = alpha (g_r u^T + G W);  P = W dW^T W;  dL = -tril(P);  Phi = sym(tril(L^T dL), diag/2);
    // dK = W Phi W^T;  E_psi = dK o K_uu.  Temporaries: Asum (G sym), Gs (T1), gsum (dW), P1, KGK, GamSum
    HIP_TRY(hipMemcpy2DAsync(g.Asum, msq * sizeof(double), g.Gsum, gstride * sizeof(double), msq * sizeof(double), Dl,
                             hipMemcpyDeviceToDevice, s));
    launch_symmetrize(s, g.Asum, Mp, Dl);
    const AtbArgs ap = mm_args(h);
    mm(s, ap, g.Asum, msq, W, kstride, g.Gs);                                           // T1 = G W
    launch_dw_a(s, g.Gs, g.Gsum + msq, gstride, g.ucol, p.log_Q, Mp, Dl, c.d_begin, g.gsum);   // dW
    mm(s, ap, g.gsum, msq, W, kstride, g.P1);                                           // Q1 = dW^T W
    mm(s, ap, h->Linv, msq, g.P1, msq, g.KGK);                                          // P = W Q1
    launch_tril_neg(s, g.KGK, Mp, Dl, g.GamSum);                                        // dL
    launch_tril_copy(s, h->Kuu, kstride, Mp, Dl, g.Lclean);
    mm(s, ap, g.Lclean, msq, g.GamSum, msq, g.P1);                                      // S = L^T dL
    launch_phi(s, g.P1, Mp, Dl, g.KGK);                                                 // Phi
    mm(s, ap, g.KGK, msq, h->Linv, msq, g.P1);                                          // Q2 = Phi W^T
    mm(s, ap, h->Linv, msq, g.P1, msq, g.KGK);                                          // dK = W Q2
    launch_epsi_a(s, kind, g.KGK, h->Kcopy, c.M, Mp, Dl, c.jitter, g.Epsi);
    enqueue_kuu_reduce(h, s);
    // du = W^T g_r (per dim) for dU
    launch_matvec(s, h->Linv, msq, g.Gsum + msq, gstride, Mp, g.du, 1, Mp, Mp, Dl);
    // K_fu side: E = (alpha K_fu K^-1 + alpha r beta^T) o K_fu, reduced in the fused kernel
    launch_scale_kinv(s, h->Kinv, p.log_Q, Mp, Dl, c.d_begin, g.GammaA);
    EReduceArgs er = grad_efu_args(h, h->F, g.beta);
    er.u_per_dim = 1;                                   // beta is per latent dim
    launch_e_product(h, s, er, h->F, g.GammaA, g.beta, g.r);
    launch_e_finish(s, er, g.dz_unit, g.dll_unit, g.dls_unit);
    const DxArgs dx = grad_dx_args(h, S_total);
    launch_dx(s, dx);
    launch_shared_partials(s, dx, g.shared_part, g.sp_stride);
    GradFinalArgs gf = grad_final_args(h, S_total);
    // dl/dalpha per unit replaces the collapsed formula, and U has a gradient: dU from du_dim
    gf.branch_a = 1; gf.dalpha_unit = g.dalpha; gf.du_dim = g.du; gf.U = p.U; gf.dU = g.dU;
    launch_fill(s, g.dlogvar, g.small_count, 0.0);        // dlogvar | dloglen | dlogQ | dCC | dDD | dlogR
    launch_grad_finalize(s, gf);
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}

int ffvd::enqueue_grad_b(ffvd_handle *h, int S_total) {
    const ffvd_config &c = h->cfg;
    ffvd_handle::GradWs &g = h->gw;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl, nb = h->nbatch, S = c.S_local;
    const size_t msq = (size_t)Mp * Mp, hstride = (size_t)(2 * Mp + NB) * Mp;
    hipStream_t s = h->stream;
    const ffvd_params &p = h->cur;
    const size_t kstride = (size_t)2 * Mp * Mp;
    const bool wh = g.whitened;
    // Reference route (F = K_fu L^-T, H = F^T F / Q + I factorised by the forward pass; fp64 or fp32 contractions): the slab already
    // holds the factor of the whitened H, so the M x M side below is the whitened one as it stands; what differs is where K_fu
    // lives (Kf2, or the fp32 copy), that sum_s H_s is read instead of W^T (sum_s A_s) W, and where sum_t |F_t|^2 comes from.
    const bool ref = c.route == FFVD_ROUTE_REFERENCE;
    const bool f32c = c.dtype == FFVD_F32C;
    const double *Kf64 = ref ? h->Kf2 : h->F;
    // explicit form: u = A^-1 c = L_A^-T (L_A^-1 c), Gamma = alpha/2 (K^-1 - A^-1 - u u^T) with A^-1 from the factor of A.
    // whitened form (default): the slab holds the factor of H = W^T A W and y = L_H^-1 b.  Then w = H^-1 b, u = W w, and
    // A^-1 = B^T B with B = L_H^-1 L^-1 (a product of two accurate triangular factors; K^-1 = (L^-1)^T L^-1 is formed
    // the same way in the forward pass), so the same Gamma launch runs on B instead of on the inverse factor of the
    // ill-conditioned A -- dZ at M = 512 then agrees with central differences to 7 digits instead of 3.
    AtbArgs ag{};
    ag.mode = ATB_GAMMA; ag.a_stride = msq; ag.lda = Mp; ag.nA = Mp;
    ag.b_stride = msq; ag.ldb = Mp; ag.nB = Mp; ag.b_per_dim = 0; ag.rows = Mp;
    ag.C = g.Gamma; ag.c_stride = msq; ag.ldc = Mp; ag.nb = nb; ag.b0 = 0; ag.Dl = Dl; ag.d_begin = c.d_begin;
    ag.log_Q = p.log_Q; ag.u = g.u; ag.u_stride = Mp; ag.Kinv = h->Kinv; ag.Kcopy = h->Kcopy; ag.k_stride = msq; ag.ldk = Mp;
    ag.part = g.gam_part; ag.k_lower = 1; ag.sym = 1; ag.small_tiles = 1;   // inverse factor lower triangular, its Gram symmetric
    // K_uu side, first half: K^-1 (sum_s A_s - S K) K^-1 needs the saved A-matrices and the K_uu chain only, not Gamma.  When the E
    // product is short (tiny problems: the side stream's launches are the critical path of the backward pass) it starts here,
    // ahead of w / u / B / Gamma; Gamma's sum joins it through ev_go.
    hipStream_t sk = h->sw.grad_serial ? s : h->aux;
    const bool tiny = (size_t)nb * Tp * Mp <= (size_t)64 * 1024 * 128 && sk != s;
    auto kgk_chain = [&]() -> int {
        launch_chain_sum(sk, g.Acopy, msq, S, Dl, msq, g.Asum, msq);      // (reference route: the saved matrices are the H_s)
        launch_symmetrize(sk, g.Asum, Mp, Dl);
        if (!ref) launch_axpby(sk, g.Asum, h->Kcopy, 1.0, -(double)S, p.log_Q, c.d_begin, 0, msq, Dl, g.Gs);
        const AtbArgs ap = mm_args(h);
        const double *W = h->Kuu + msq;                                 // L^-T rows, per dim stride kstride
        if (wh) {       // K^-1 Gs K^-1 = W (W^T Gs W) W^T, conjugated step by step (Gs and W^T Gs W are symmetric)
            if (ref) launch_sub_identity(sk, g.Asum, (double)S, Mp, Dl, g.P2);     // W^T Gs W = sum_s (H_s - I): no products needed
            else {
                mm(sk, ap, g.Gs, msq, W, kstride, g.P1, 8);         // P1 = Gs W
                mm(sk, ap, W, kstride, g.P1, msq, g.P2, 4);         // P2 = W^T Gs W
            }
            mm(sk, ap, g.P2, msq, h->Linv, msq, g.P3, 2);           // P3 = P2 W^T
            mm(sk, ap, h->Linv, msq, g.P3, msq, g.KGK, 1);          // KGK = W P3
        } else {
            mm(sk, ap, g.Gs, msq, h->Kinv, msq, g.P1);              // P1 = Gs^T K^-1 = Gs K^-1
            mm(sk, ap, g.P1, msq, h->Kinv, msq, g.KGK);             // P1^T K^-1 = K^-1 Gs K^-1
        }
        return FFVD_OK;
    };
    if (tiny) {
        { int rcf = fork_side(h, h->ev_fork, s, sk); if (rcf) return rcf; }
        kgk_chain();
    }
    if (wh) {
        launch_matvec(s, h->H + msq, hstride, h->H + 2 * msq, hstride, Mp, g.wv, 1, Mp, Mp, nb);          // w = L_H^-T y
        launch_matvec(s, h->Kuu + msq, kstride, g.wv, Mp, Mp, g.u, 1, Mp, Mp, nb, Dl);                     // u = W w
        AtbArgs tb{};       // B[i][j] = sum_k L_H^-T[k][i] L^-1[k][j]: the extension rows as they are, no transpose
        tb.mode = ATB_PLAIN; tb.A = h->H + msq; tb.a_stride = hstride; tb.lda = Mp; tb.nA = Mp;
        tb.B = h->Linv; tb.b_stride = msq; tb.ldb = Mp; tb.nB = Mp; tb.b_per_dim = 1; tb.rows = Mp;
        tb.C = g.T1; tb.c_stride = msq; tb.ldc = Mp; tb.nb = nb; tb.Dl = Dl; tb.krange = 2 | 4; tb.small_tiles = 1;      // k in [tile tj, tile (ti + 1))
        launch_atb(s, tb);
        ag.A = g.T1; ag.B = g.T1;
    } else {
        launch_matvec(s, h->H + msq, hstride, h->H + 2 * msq, hstride, Mp, g.u, 1, Mp, Mp, nb);
        launch_transpose(s, h->H + msq, hstride, g.LAinv, msq, Mp, nb);
        ag.A = g.LAinv; ag.B = g.LAinv;
    }
    launch_atb(s, ag);
    DBG_SYNC(h, "backward: w, u, B, Gamma");
    // K_uu side: Psi_d = sum_s Gamma_s / alpha_d - 1/2 K^-1 (sum_s A_s - S K) K^-1.  It needs Gamma and the saved
    // A-matrices only, so its dozen small launches go to the side stream and run beside the E product
    // (enqueued after it: the main stream must not wait for their launch overhead).
    if (sk != s) { int rcf = fork_side(h, tiny ? h->ev_go : h->ev_fork, s, sk); if (rcf) return rcf; }          // Gamma is there
    EReduceArgs er = grad_efu_args(h, Kf64, g.u);
    const int kind = c.kernel_kind;
    if (kind != FFVD_KERNEL_SE) launch_xsq_unit(sk, p.X, h->ctrl, c.T, c.D, c.C, S, Dl, g.xsq);
    launch_e_product(h, s, er, Kf64, g.Gamma, g.u, nullptr);
    DBG_SYNC(h, "backward: E product + reductions");
    launch_e_finish(s, er, g.dz_unit, g.dll_unit, g.dls_unit);
    DBG_SYNC(h, "backward: e_finish");
    // latent trajectories (after the E product) and the per-chain partials of the shared parameters (inputs only: side)
    const DxArgs dx = grad_dx_args(h, S_total);
    // u^T K u and the per-chain partials of the shared parameters feed grad_finalize only.  Beside a long E product they ride on
    // the side stream; when that product is a few dozen microseconds (the reference's own experiment sizes) the side stream's
    // dozen launches ARE the backward pass's critical path and these two go to the main stream, which has the slack there
    hipStream_t su = ((size_t)nb * Tp * Mp <= (size_t)64 * 1024 * 128 && !h->sw.grad_serial) ? s : sk;
    if (wh) launch_utu(su, g.wv, Mp, Mp, nb, g.uku);                       // u^T K u = w^T w
    else launch_uku(su, g.u, Mp, h->Kcopy, msq, Mp, Dl, nb, g.uku);   // u^T K u per unit: only grad_finalize reads it
    launch_shared_partials(su, dx, g.shared_part, g.sp_stride);
    if (!tiny) kgk_chain();
    launch_chain_sum(sk, g.Gamma, msq, S, Dl, msq, g.GamSum, msq);
    launch_axpby(sk, g.GamSum, nullptr, 1.0, 0.0, p.log_Q, c.d_begin, 1, msq, Dl, g.gsum);
    launch_psi_e(sk, g.gsum, g.KGK, h->Kcopy, c.M, Mp, Dl, c.jitter, g.Epsi, kind);
    enqueue_kuu_reduce(h, sk);
    if (sk != s) HIP_TRY(hipEventRecord(h->ev_join, sk));
    if (sk != s) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
    DBG_SYNC(h, "backward: K_uu side");
    launch_dx(s, dx);
    GradFinalArgs gf = grad_final_args(h, S_total);
    // U is integrated out: the collapsed formula's traces, forward terms and u^T K u per unit
    gf.gam_part = g.gam_part; gf.ngam = g.ngam; gf.trpart = h->trpart; gf.ntr = h->ntiles; gf.hterms = h->hterms; gf.uku = g.uku;
    if (ref) { gf.trpart = f32c ? h->sqsum : g.fsq; gf.ntr = 1; }       // sum_t |F_t|^2 per unit (Gram route: tr(K^-1 K_uf K_fu) by tiles)
    // entries this handle does not own (other ranks' dims; the shared terms off rank 0) stay zero for the all-reduce
    launch_fill(s, g.dlogvar, g.small_count, 0.0);        // dlogvar | dloglen | dlogQ | dCC | dDD | dlogR
    launch_grad_finalize(s, gf);
    DBG_SYNC(h, "backward: dx + finalize");
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}

int ffvd::enqueue_grad(ffvd_handle *h, int S_total) {
    return h->cfg.branch == FFVD_BRANCH_A ? enqueue_grad_a(h, S_total) : enqueue_grad_b(h, S_total);
}

// the gradient arrays of the handle to the caller's host arrays (enqueued on the main stream; the caller synchronises)
int ffvd::copy_grads_out(ffvd_handle *h, const ffvd_grads *gout) {
    const ffvd_config &c = h->cfg;
    ffvd_handle::GradWs &g = h->gw;
    hipStream_t s = h->stream;
    const size_t P = h->P, J = c.Ydim;
    if (gout->X) HIP_TRY(hipMemcpyAsync(gout->X, g.dX, (size_t)c.S_local * (c.T + 1) * c.D * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->Z) HIP_TRY(hipMemcpyAsync(gout->Z, g.dZ, (size_t)c.M * P * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->logvariance) HIP_TRY(hipMemcpyAsync(gout->logvariance, g.dlogvar, (size_t)c.D * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->loglengthscales) HIP_TRY(hipMemcpyAsync(gout->loglengthscales, g.dloglen, (size_t)c.D * P * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->log_Q) HIP_TRY(hipMemcpyAsync(gout->log_Q, g.dlogQ, (size_t)c.D * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->CC) HIP_TRY(hipMemcpyAsync(gout->CC, g.dCC, (size_t)c.D * J * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->DD) HIP_TRY(hipMemcpyAsync(gout->DD, g.dDD, J * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->log_Rchols) HIP_TRY(hipMemcpyAsync(gout->log_Rchols, g.dlogR, J * J * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gout->U) {
        if (g.dU) HIP_TRY(hipMemcpyAsync(gout->U, g.dU, (size_t)c.M * c.D * sizeof(double), hipMemcpyDeviceToHost, s));
        else memset(gout->U, 0, (size_t)c.M * c.D * sizeof(double));        // collapsed branch: U is integrated out
    }
    return FFVD_OK;
}
