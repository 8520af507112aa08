// Gauss-Newton polish of the map-joining objective: what its files share.
//   lsfm_gn_structure.cpp   the joint system's structure from labels, on the host (GnStructure)
//   lsfm_gn.hip             gn_begin (arenas, the batch, the structure, gn_upload of its arrays), the polish loop, lsfm_map_chi2 / lsfm_map_feature_chi2 /
//                           lsfm_gn_linearise
//   lsfm_gn_assemble.hip    one assembly at the state in d_x: its kernels and gn_assemble
//   lsfm_gn_chi2.hip        chi^2 per map and per feature, the robust weights and objective, the feature weights' correction of U
#pragma once
#include <algorithm>

#include "lsfm_gn_structure.hpp"
#include "lsfm_internal.hpp"

namespace lsfm {

struct GnMap : GnMapShape {
	double w; // weight of the map's information matrix in the step (1 unless the robust polish re-weights it: k_gn_robust_weights)
	// the frame at the current state (k_gn_hubs)
	double R[9], dRA[9], dRB[9], dRG[9], t[3];
	double Scale, Scale2, dSdt[3], dSdtt[3], dSdA, dSdB, dSdG; // (row Fix_k of the reference's dSdt / dSdtt, component Fix_k of dSdA..)
};
#define GN_GW 78 /* pose row of G = I [C_1 C_2 r]: 36 + 36 + 6 */
#define GN_HW 121 /* per map: C_1^T G_1, C_1^T G_2, C_2^T G_2 (36 each), C_1^T g, C_2^T g (6 each), r^T g */
inline dim3 gn_grid(size_t n, int b) { return dim3((unsigned)std::max<size_t>(1, (n + b - 1) / b)); }

// the U list an assembly and the chi^2 read: the batch's own, or the extended one (every map's blocks followed by its correction slots)
struct GnUView { const double* U = nullptr; const int *Ui = nullptr, *Uj = nullptr; int NU = 0; };
// lsfm_map_feature_chi2 / lsfm_gn_polish_robust_features / lsfm_gn_linearise_features only: the per-feature arrays and, for the polish
// and the linearisation, the correction slots of U
struct GnFeat {
	int NS = 0;           // correction slots over all maps
	size_t NC = 0;        // contributors over all slots
	double* Ux = nullptr; // the extended list's blocks (what GnCall::u views): own blocks copied once, slots filled by every assembly
	int *d_sptr = nullptr, *d_cf = nullptr, *d_ca = nullptr, *d_cb = nullptr, *d_eptr = nullptr, *d_eidx = nullptr, *d_sdst = nullptr, *d_bad = nullptr;
	double *fchi2 = nullptr, *fw = nullptr, *msum = nullptr, *pose_chi2 = nullptr;
};
// lsfm_gn_linearise[_features] only: the sources of every output block (CSR) and the output blocks
struct GnCoalesceDev { int *d_wsp = nullptr, *d_wsi = nullptr, *d_usp = nullptr, *d_usi = nullptr; double *Wo = nullptr, *Uo = nullptr; };
// what gn_upload leaves on the device for the call's steps: the uploaded local maps, the joint system's structure, the work arrays
struct GnCall {
	int N = 0, M = 0, NFG = 0, P = 0, FI = 0, NUJ = 0, NWJ = 0;
	size_t RS = 0; // scalars of the global state
	bool mono = false;
	DevBatch X;
	GnUView u;
	GnMap* d_gm = nullptr;
	int *d_gp = nullptr, *d_gf = nullptr, *d_wdst = nullptr, *d_fptrJ = nullptr, *d_photoJ = nullptr, *d_fsp = nullptr, *d_fsi = nullptr, *d_psp = nullptr,
	    *d_psi = nullptr, *d_UiJ = nullptr, *d_UjJ = nullptr, *d_org = nullptr, *d_seg = nullptr;
	unsigned char* d_fixed = nullptr;
	double *d_x = nullptr, *d_x0 = nullptr, *d_dl = nullptr, *Dp = nullptr, *Cp = nullptr, *rp = nullptr, *Gacc = nullptr, *Hacc = nullptr, *Fsum = nullptr;
	double *ePinst = nullptr, *Vinst = nullptr, *eFinst = nullptr, *UJ = nullptr, *WJ = nullptr, *VJ = nullptr, *ea = nullptr, *eb = nullptr;
	unsigned long long* d_max = nullptr;
	double *d_chi2 = nullptr, *d_G = nullptr; // [N] chi2_k (k_gn_chi2<false>); the robust objective G of either estimator
	int* d_dof = nullptr;                     // the estimator on the maps: [N] dof_k and the weights w_k
	double* d_w = nullptr;
	GnFeat feat;      // the estimator on the features, and lsfm_map_feature_chi2
	GnCoalesceDev co; // lsfm_gn_linearise
};
// what a call needs beyond the plain polish's arrays: the per-feature arrays, the correction slots of U, the coalesced form
struct GnWants {
	bool feat = false, slots = false, coalesce = false;
	static GnWants feature_chi2() { GnWants w; w.feat = true; return w; }
	static GnWants polish_features() { GnWants w; w.feat = w.slots = true; return w; }
	static GnWants linearise() { GnWants w; w.coalesce = true; return w; }
	static GnWants linearise_features() { GnWants w; w.feat = w.slots = w.coalesce = true; return w; }
};
// what is re-weighted, and how: kind 1 Huber, 2 Cauchy with threshold c on chi2_k / dof_k (maps) or c_kf / 3 (features).  given
// (lsfm_gn_linearise_features): no estimator -- the feature weights are what the caller uploaded into GnFeat::fw, and the maps' weights
// those of gn_upload; kind and c are unused
struct GnEstimator { enum On { none, maps, features, given } on = none; int kind = 0; double c = 1.0; };
// LSFM_GN_TIMING: events recorded around the chi2 + weights launches and around the fill of the correction slots
struct GnEvents { hipEvent_t chi2[2] = { nullptr, nullptr }, fill[2] = { nullptr, nullptr }; };

// ---- lsfm_gn_assemble.hip ----
// the frames of the maps at the state in d_x, the pose residuals r_a with their D_a and C_s,a
void gn_frames(lsfm_context* ctx, const GnCall& c);
// the launches of one assembly at the state in d_x: F into Fsum, the joint system UJ / WJ / VJ and the right-hand sides ea / eb.
// est.on == maps: the robust weights first (G into d_G).  features: the feature chi2 pass (G into d_G), the correction slots of U, W and
// V weighted per feature; the maps' own weights stay as gn_upload left them.  given: as features with the weights in feat.fw read, not
// written, and d_G = sum_k w_k (pose_chi2_k + sum_f w_kf c_kf).  ev (may be null): recorded around those parts.
void gn_assemble(lsfm_context* ctx, const GnCall& c, const GnEstimator& est, const GnEvents* ev);
// ---- lsfm_gn_chi2.hip (all after gn_frames) ----
// chi2_k of every map into d_chi2; then s_k = chi2_k / dof_k, the weights w_k = rho'(s_k) into the maps' frames and d_w, G into d_G
void gn_map_chi2(lsfm_context* ctx, const GnCall& c);
void gn_map_weights(lsfm_context* ctx, const GnCall& c, int kind, double cth);
// c_kf, w_kf and the per-map sums at the state in d_x, then pose_chi2 and G into d_G (kind 0: every weight 1)
void gn_feature_chi2(lsfm_context* ctx, const GnCall& c, int kind, double cth);
// the same pass with the weights w_kf given in feat.fw (read only): c_kf, the per-map sums, the report of a V that is not positive
// definite, pose_chi2 and d_G = sum_k w_k (pose_chi2_k + sum_f w_kf c_kf) with the maps' weights of gn_upload
void gn_feature_chi2_given(lsfm_context* ctx, const GnCall& c);
// the maps' own U blocks into the extended list (once per call) / its correction slots from the feature weights (every assembly)
void gn_extend_u(lsfm_context* ctx, const GnCall& c, const int* d_ushift);
void gn_feature_ufill(lsfm_context* ctx, const GnCall& c);

} // namespace lsfm
