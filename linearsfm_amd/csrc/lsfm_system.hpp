// One system I = [U W; W^T V] handed over in host arrays (C ABI: lsfm_solve_*, lsfm_map_covariance[_columns], lsfm_map_marginalise,
// lsfm_schur_pattern): the checks of its index arrays and its way into arena 0, once for every entry point.
// The checks are plain C++ (lsfm_system.cpp, compiled by g++ like lsfm_symbolic.cpp: callable without a device); the upload is
// lsfm_system.hip.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/lsfm.h"

struct lsfm_context;

namespace lsfm {

struct SolveIO;

// the system as the caller holds it; the value arrays may be null where the call does not ask for them
struct HostSystem {
	int m = 0, n = 0, nU = 0, nW = 0;
	const int *Ui = nullptr, *Uj = nullptr, *photo = nullptr, *feature = nullptr;
	const double *U = nullptr, *W = nullptr, *V = nullptr;
	const double *ea = nullptr, *eb = nullptr, *x0 = nullptr; // [6 m] / [3 n] right-hand sides, [6 m] initial guess
	const int* pose_origin = nullptr;                        // [m]
};
// the system of a map: its sizes and index arrays, and (values) U, W, V; the right-hand sides and pose_origin stay unset
inline HostSystem host_system_of(const lsfm_map& g, bool values)
{
	HostSystem h;
	h.m = g.m; h.n = g.n; h.nU = g.nU; h.nW = g.nW;
	h.Ui = g.Ui; h.Uj = g.Uj; h.photo = g.photo; h.feature = g.feature;
	if (values) { h.U = g.U; h.W = g.W; h.V = g.V; }
	return h;
}

// ---- host only (lsfm_system.cpp) ----
// fptr[n + 1]: the W run of every feature, from feature[] (W sorted by feature); 0 <= Ui <= Uj < m; 0 <= photo < m.
// LSFM_OK, or LSFM_ERR_ARG with *why = what is wrong.  empty_features_ok: a feature without a W block is let through (the pattern
// of S alone has a use for it; everything that inverts V per feature has not).
int system_check(const HostSystem& h, bool empty_features_ok, std::vector<int>& fptr, const char** why);
// the gauge mask fixed[6 m]: 1 = scalar removed from the system -- the 6 scalars of pose `blk` and scalar `scalar` (either < 0 or out
// of range: none)
std::vector<unsigned char> gauge_mask(int m, int blk, int scalar);

// ---- device (lsfm_system.hip) ----
// system_check for an entry point: fptr, or an Error (LSFM_ERR_ARG) with its message
std::vector<int> system_fptr(const HostSystem& h, bool empty_features_ok = false);
enum SystemPieces : unsigned {
	SYS_VALUES  = 1u << 0, // U, W, V (without: the index arrays alone -- the pattern of S)
	SYS_RHS     = 1u << 1, // ea / eb from the host arrays, and the segment arrays of the one system
	SYS_RHS_0   = 1u << 2, // ... zeros instead (the right-hand side is not used)
	SYS_X       = 1u << 3, // x0 (where given) and the outputs x_pose / x_feat
	SYS_FEATURE = 1u << 4, // feature[] of every W block on the device as well
	SYS_OFFSETS = 1u << 5, // d_pose_off / d_feat_off / d_u_off of the one system: { 0, m }, { 0, n }, { 0, nU }
};
// what ensure_arenas is asked for on behalf of one system
size_t system_arena_need(const HostSystem& h, unsigned pieces);
// sizes (and resets) arena 0 and the scratch arena, uploads the pieces asked for -- pose_origin and the mask `fixed` where they are
// given -- and fills io: one system, nseg = 1, seg_rows = { m }.  d_feature (may be null): where SYS_FEATURE went.
void system_upload(lsfm_context* ctx, const HostSystem& h, unsigned pieces, const std::vector<int>& fptr, const std::vector<unsigned char>* fixed,
                   SolveIO& io, const int** d_feature = nullptr);

} // namespace lsfm
