// Marginalising features out of a map on the device (lsfm_marg.hip): what the host entry (lsfm_map_marginalise) and the reduced pack of
// a resident result (lsfm_tree_export_reduced_*) share.
#pragma once
#include "lsfm_internal.hpp"
#include "lsfm_marg_poses.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

// a map resident on the device, indices local to it (a SolveIO-style view plus feature[] of every W block)
struct MargView {
	int M = 0, NF = 0, NU = 0, NW = 0;
	const double* U = nullptr; const int *Ui = nullptr, *Uj = nullptr;
	const double* W = nullptr; const int *photo = nullptr, *feature = nullptr, *fptr = nullptr;
	const double* V = nullptr;
	const double* feat = nullptr; // [NF * 3] estimates and [NF] labels of the features (null: the kept features are not gathered)
	const int* feat_id = nullptr;
};
// where the kept features go (device; all null: the caller compacts them itself and only the dropped blocks move)
struct MargKept {
	double *W = nullptr, *V = nullptr, *feat = nullptr;
	int *photo = nullptr, *feature = nullptr, *fptr = nullptr, *feat_id = nullptr;
};
// the state of one reduction between its two halves; everything lives in `ar` and the scratch arena
struct MargWork {
	MargView in;
	const int* drop = nullptr;     // [NF + 1] 1: marginalised out (entry NF: 0)
	int *kpos = nullptr, *kwpos = nullptr; // [NF + 1] exclusive scans of the kept flags / the kept run lengths
	int nkeep = 0, nWkeep = 0, ndrop = 0, nWdrop = 0;
	int *dfp = nullptr, *dph = nullptr; // run pointers [ndrop + 1] and poses [nWdrop] of the dropped features, made contiguous
	SolveIO io;                    // K9's input: U and the dropped features
	SchurSystem sy;                // sy.nnzb / sy.upper_keys: the pattern of U'
};
// drop[f] = 1 unless feat_id[f] is in the sorted list keep[0..nkeep)
void marg_flags_from_keep(lsfm_context* ctx, int NF, const int* feat_id, const int* keep_sorted, int nkeep, int* drop);
// first half: positions from the flags, the dropped runs' index arrays, the pattern of U'.  nkeep / nWkeep < 0: counted on the device
// and read back (one synchronisation); the pattern build synchronises once more.
void marg_structure(lsfm_context* ctx, Arena& ar, const MargView& in, const int* drop, int nkeep, int nWkeep, MargWork& w);
// second half: the one partition pass over W, the per-feature gather, V^-1 of the dropped features, K9, and U' / Ui / Uj (device,
// sy.nnzb blocks).  d_err (device int, zeroed by the caller): != 0 afterwards = a dropped V block was not positive definite.
// ev (may be null): [3] events recorded behind the partition pass, behind the gather + V^-1 and behind K9's values.
void marg_values(lsfm_context* ctx, Arena& ar, MargWork& w, const MargKept& kept, double* oU, int* oUi, int* oUj, int* d_err, hipEvent_t* ev);
// lsfm_tree_export_reduced_*: the reduced pack of the single map of `b` (a finished tree's final map), its features cut down to the
// labels keep_ids[0..nkeep).  ar: work space, an arena the map does not live in (reset here).  dst == null: the size alone, to *bytes.
// times (may be null): [5] ms of structure | partition pass | gather + V^-1 | K9 values | emit
void marg_export_reduced(lsfm_context* ctx, const DevBatch& b, bool mono, Arena& ar, const int* keep_ids, int nkeep, void* dst, size_t cap, size_t* bytes,
                         double* times);
// lsfm_map_marginalise
int map_marginalise(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out, double* times);
// lsfm_map_marginalise_poses (lsfm_marg_poses.hip; the structure: lsfm_marg_poses.hpp): stage A = map_marginalise over the features that
// go with the dropped poses, then U'_KK = U1_KK - Y^T Y from a forward sweep against the factor of U1_DD.  times (may be null): [5] ms of
// stage A | structure + upload | factor | right-hand sides + sweeps | SYRK + emit + download; info (may be null): [8] = |D|, |Bd|,
// components, output blocks, chunks, leaf tasks, supernode groups, group levels.  > 0: floored pivots, nothing written.
int map_marginalise_poses(lsfm_context* ctx, const lsfm_map* map, bool mono, const unsigned char* keep_pose, const unsigned char* drop_feat, lsfm_map* out,
                          double* times, int* info);

} // namespace lsfm
