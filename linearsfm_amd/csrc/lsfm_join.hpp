// Shared by the Stereo and the Mono join (lsfm_join.hip, lsfm_join_mono.hip).
#pragma once
#include "lsfm_internal.hpp"

namespace lsfm {

struct JGroup {
	int F0E, nE, F0C, nC; // feature ranges of End / Cur in the input batch (nC = 0: carried map)
	int FY0;              // first joint feature
	int rC0;              // rank offset of Cur's unmatched features
};

// state of a Stereo join between its two steps (lsfm_join.hip)
struct JoinState {
	size_t smark = 0;
	int *newf = nullptr, *lenE = nullptr, *srcf = nullptr, *wbase = nullptr;
	double *eP = nullptr, *eF = nullptr;
	std::vector<unsigned char> seg_active, act_padded;
	unsigned char* d_act = nullptr; // device copy of seg_active
	std::vector<int> seg_rows;
	bool fuse_rhs = false;                    // the W part of the right-hand sides goes with the Schur assembly (RhsFused)
	int *srcE = nullptr, *srcC = nullptr;     // per joint feature its sources in the input batch (-1: none)
};
// level_in, hub: a tree level reached through the transform's hook -- the level's input (before the transform) and the hub pose of
// every transformed map (TrHook), from which a level that analyses starts the early pattern of S; null: no early pattern
void join_stereo_prepare(lsfm_context* ctx, Arena& ar, const DevBatch& in, DevBatch& out, JoinState& st, const DevBatch* level_in, const int* hub);
// step_hint: SolveIO::step_hint of the solve, whose outcome is returned
SolveOutcome join_stereo_finish(lsfm_context* ctx, const DevBatch& in, DevBatch& out, JoinState& st, double* eP_out, double* eF_out, int step_hint = 0);

// ---- what a join of either kind is made of ----
// match[f] = feature of the pair's first map with the same label (-1 none), unm[f] = 1 for unmatched features of the
// second map (unm[NF] = 0)
void join_match_features(lsfm_context* ctx, const DevBatch& in, int* match, int* unm);
// the same from scratch memory, with the ranks of the unmatched features: match[NF + 1], R[NF + 2] = exclusive scan of unm.  R at the
// map boundaries (k_gather_at with in.d_feat_off) is `rb` below
struct JoinRanks { int *match, *R; };
JoinRanks join_rank_features(lsfm_context* ctx, const DevBatch& in);
// The joint maps of a level, on the host: pair g joins maps 2g (End) and 2g + 1 (Cur) of the B input maps, the last map of an odd level
// is carried as it is.  feat_off / pose_off: the input's; rb: [B + 1] ranks of the unmatched features at the map boundaries (Cur's
// unmatched features follow End's features); shared: poses of Cur that a pair holds once because they are End's too (Stereo 0, Mono 2:
// Imp.cpp:7309-7314).  Fills grp, out.feat_off, out.pose_off, the pose rows of every joint map and whether it is a pair
void join_layout(int B, const std::vector<int>& feat_off, const std::vector<int>& pose_off, const std::vector<int>& rb, int shared, DevBatch& out,
                 std::vector<JGroup>& grp, std::vector<int>& seg_rows, std::vector<unsigned char>& seg_active);
// the joint maps `out` as the system of solve_batch: sizes, segments, blocks and their indices, right-hand sides eP / eF, where the state
// goes, and the ranges of the joins for a level of small systems (small_level_offsets).  The first guess, the gauge and RhsFused /
// PatternSeed are the caller's
SolveIO join_solve_io(lsfm_context* ctx, const DevBatch& out, const unsigned char* d_act, const double* eP, const double* eF,
                      const std::vector<int>& seg_rows, bool at_evA, int step_hint);
// the end of a join: scratch back to smark, systems left above their bound into the stats, the level's plan valid (whole_level: not
// a stage-level call that had the right-hand sides copied out).  Waiting for the stream, where a join must, comes before
void join_close(lsfm_context* ctx, size_t smark, const SolveOutcome& oc, bool whole_level);
__global__ void k_gather_at(const int* __restrict__ src, const int* __restrict__ idx, int n, int* __restrict__ out);
__global__ void k_join_features(int NF, const int* __restrict__ feat_map, const int* __restrict__ feat_id, const double* __restrict__ feat,
                                const double* __restrict__ V, const int* __restrict__ fptr, const int* __restrict__ match,
                                const int* __restrict__ R, const JGroup* __restrict__ grp, int* __restrict__ newf, int* __restrict__ lenE,
                                int* __restrict__ lenC, double* __restrict__ Vy, double* __restrict__ eF, int* __restrict__ fid_y,
                                double* __restrict__ feat_y, int* __restrict__ srcE, int* __restrict__ srcC, int side);

} // namespace lsfm
