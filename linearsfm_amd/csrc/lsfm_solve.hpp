// Shared between lsfm_pattern.hip (the pattern of S), lsfm_solve.hip (Schur assembly, SpMV, back-substitution), lsfm_level.hip (the
// level driver), lsfm_chol.hip (the factorisation) and lsfm_pcg.hip (the refinement).
#pragma once
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"

// features per tile of K9's panel kernel (lsfm_schur_panel.hip); the per-feature fallback k_schur_w keeps tiles of 128 and looks its
// flag up in the panel kernel's tiling
#ifndef LSFM_PM_TILE
#define LSFM_PM_TILE 128
#endif

namespace lsfm {

// What K9's panel kernel works out per tile of 128 features from index arrays alone (which poses see the tile = its slots,
// the slot of every W block, which blocks repeat a (pose, feature) pair): recorded by the first run of a resident tree,
// read by the later ones instead of hashing the tile's poses again.  ns[tile] = -1: no panel variant takes the tile.
struct K9Cache {
	int* ns = nullptr;            // [tiles]
	int* pose = nullptr;          // [tiles * 64]
	unsigned char* eslot = nullptr; // [NW]
	int* wlist = nullptr;         // [3 * tiles] tiles of the 32- / 48- / 64-slot variants, wcnt[v] of them each
	int* wcnt = nullptr;          // [8]: [0..2] tiles in the lists (structure, kept by a plan), [4..6] the cursors of a launch
};

struct SchurSystem {
	int M = 0, nnzb = 0;
	int *rowptr = nullptr, *colidx = nullptr;      // upper block CSR (diagonal block first in every row)
	const unsigned long long* upper_keys = nullptr; // [nnzb] sorted (row << 32 | col) of the upper pattern
	double* S = nullptr;                           // [nnzb*36]
	double* E = nullptr;                           // [M*6]
	double* IV = nullptr;                          // [NF*9]
	double* LY = nullptr;                          // [NF*9] Cholesky factor of V^-1 (6) and L^T eb (3) per feature, for K9's panel kernel
	int* longrows = nullptr;        // rows with more than SP_LONG blocks (hub poses), *d_nlong of them
	const int* d_nlong = nullptr;
	// cache-resident matrices: both orientations of every block sorted by the row they contribute to (k_spmv_gather);
	// 2 nnzb slots, the holes of the diagonal blocks (~0) at the end; null for a matrix that streams from HBM (k_spmv)
	const unsigned long long* gent = nullptr;
	const int* goth = nullptr;
	const unsigned long long* tab = nullptr; // pose pair -> block of S (open addressing), values in hval
	const int* hval = nullptr;
	unsigned long long mask = 0;
	// K9's sums in fixed point (lsfm_device.hpp "order-independent sums"): acc = one poison word, then [nnzb * 36] accumulators of
	// W V^-1 W^T, then [6 M] high and [6 M] low limbs of the right-hand side's -W V^-1 eb; sexp = [6 M] binary exponents of the
	// pose scalars' scales (2^sexp > 2 sqrt(U_ii)) and, at [6 M], the exponent that bounds |L^T eb| over the level
	long long* acc = nullptr;
	int* sexp = nullptr;
	double* uu = nullptr;    // [NF * 6] fused right-hand side: L^-1 x_f for the End / Cur source of every feature (K9Out::uu)
	double* ymax = nullptr; // [work-groups of k_vinv] largest |L^T eb|^2 of each
	K9Cache k9;      // per-tile structure of K9 (null: every run works it out)
	int k9_tiles = 0, k9_NW = 0;
	double k9_flops = 0; // algorithmic flops of the numeric Schur complement of this system (structure only)
};

// ---- the pattern of S (lsfm_pattern.hip) ----
// The pattern of a Mono level's camera system from the one below (the Stereo levels have had this since round 3, through the early
// pattern): every pose pair inside one source map is in the level below's pattern -- a joint feature is seen by everything its
// sources were seen by --, the transform's hub links are blocks of the joint U, and what is new are the pairs ACROSS the two sources of
// a matched feature.  Poses are renumbered by the join (Cur's copies of the shared reference / scale pose become End's: pnew), and the
// blocks of the gauge-fixed reference pose are dropped (Imp.cpp:7482-7547, 7619-7700): `dropped`.
struct PatternSeed {
	const unsigned long long* prev_keys = nullptr; // sorted upper pattern of the level below, in the INPUT batch's pose numbering
	int prev_nnzb = 0;
	const int* pnew = nullptr;               // [input poses] -> joint pose
	const unsigned char* dropped = nullptr;  // [input poses] 1: a pose whose U / W blocks the join drops
	int NFY = 0;                             // joint features
	const int *srcE = nullptr, *srcC = nullptr; // [NFY] source features in the input batch (-1: none)
	const int *fptr_in = nullptr, *photo_in = nullptr; // W runs of the input batch
};
// what the early pattern is made from: X = the level's input batch (index arrays only), per joint feature its source
// features in X (srcE / srcC, -1: none), per map of X its hub pose
struct EarlyPatternIn {
	int M = 0, NFY = 0, NU = 0;
	const int *Ui = nullptr, *Uj = nullptr, *pose_map = nullptr, *hub = nullptr;
	const int *fptr = nullptr, *photo = nullptr, *feat_map = nullptr, *srcE = nullptr, *srcC = nullptr;
};
void build_schur_pattern(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy);
// the block pattern of S alone (K8), from the index members of io: upper block CSR left in the scratch arena
void schur_pattern_only(lsfm_context* ctx, const SolveIO& io, int* nnzb, const int** rowptr, const int** colidx);
void schur_pattern_early_issue(lsfm_context* ctx, const EarlyPatternIn& in); // enqueues on the side stream; the caller has recorded evC_pairs
void schur_pattern_early_drop(lsfm_context* ctx);
bool schur_pattern_early_finish(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy);
void schur_pattern_early_extras(lsfm_context* ctx, SchurSystem& sy);
bool schur_pattern_prefetch(lsfm_context* ctx, const DevBatch& Y, const int* d_tref, const unsigned long long* prev_keys, int prev_nnzb, SchurSystem& sy,
                            std::vector<int>* counts = nullptr, bool want_pattern = true, LevelIndex* keep = nullptr);
// debug / tests (LSFM_CHECK_EARLY_PATTERN, LSFM_CHECK_MONO_SEED): a pattern made ahead of the joint map (`what`: early, prefetched,
// seeded) must be the one built from the finished joint map `io` -- synchronises the device, fails unless the key lists are equal
void schur_pattern_check(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const char* what);
void rowptr_from_keys(lsfm_context* ctx, int M, int cnt, const unsigned long long* sorted_upper, int* rowptr);

void build_schur_values(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy);
void schur_vinv(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy);
void build_spmv_index(lsfm_context* ctx, SchurSystem& sy, const unsigned long long* sorted_upper);
void launch_spmv(lsfm_context* ctx, const SchurSystem& sy, const double* x, double* y, const unsigned char* fixed, const double* dotw,
                 const int* pose_seg, double* dot, int dot_stride);
double spmv_bytes(const SchurSystem& sy);
void launch_schur_slots(lsfm_context* ctx, int NF, const int* fptr, const int* photo, unsigned char* fallback, K9Cache kc);
// where K9 adds: the fixed-point accumulators of a SchurSystem and the scales they are in
struct K9Out {
	long long* S = nullptr;      // [nnzb * 36] += W V^-1 W^T in units of 2^(sexp_r + sexp_c - 60)
	long long *Ehi = nullptr, *Elo = nullptr; // [6 M] += -W V^-1 eb, two limbs: units of 2^(sexp + ey - 62) and 2^-40 of that
	long long* poison = nullptr; // != 0: an addend was not finite or outside its bound (the information matrices are not positive semi-definite)
	const int* sexp = nullptr;   // [6 M]
	const int* ey = nullptr;     // -> sexp[6 M]: 2^ey bounds |L^T eb| over the level's features
	// The W part of the join's right-hand sides taken by K9 itself (a pass over W of its own until round 5: k_join_rhs_w): non-null =
	// eb holds the V part only (k_join_features), E starts as U's part of the pose side.  With P = W L of a pass:
	//   y = L^T (eb + W^T x_p) = L^T eb + P^T x_p           (x_p: the estimates of the poses, xpose)
	//   E -= P (y - u),  u = L^-1 x_f                        (x_f: the estimate of the feature in the map the block came from:
	//                                                         uu = [u of its End source | u of its Cur source] per feature, k_vinv;
	//                                                         pside[pose] & 1 says which map a pose -- and so its blocks -- came from)
	// (lsfm_schur_panel.hip has how the panel kernel gets both out of its matrix products); the back-substitution needs no y of its
	// own: x_f = L (L^T eb - L^T sum W^T (x_p - x^_p)), k_backsub.   Imp.cpp:2770-2786, 2822-2838, 2891-2906
	const double* xpose = nullptr;
	const int* pside = nullptr;
	const double* uu = nullptr;
};
// what the fused right-hand side needs beside the joint map (lsfm_join.hip): per joint feature its sources in the level's input,
// their estimates, the poses' estimates and maps
struct RhsFused {
	const int *srcE = nullptr, *srcC = nullptr; // [NF] source feature in the input batch, -1: none
	const double* feat_src = nullptr;           // [input features * 3]
	const double* pose_src = nullptr;           // [M * 6]
	const int* pose_map_src = nullptr;          // [M] map of the input batch a pose belongs to (odd: the second map of its pair)
};
void launch_schur_panel(lsfm_context* ctx, int NF, const int* fptr, const int* photo, const double* W, const double* LY,
                        const unsigned long long* tab, const int* val, unsigned long long mask, K9Out out, unsigned char* fallback,
                        int max_poses_per_system, K9Cache kc, bool fresh_lists = false);
void launch_backsub(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const double* x);

// ---- hash set of block coordinates (pose pair -> block of S: SchurSystem::tab / hval) ----
static const unsigned long long HEMPTY = ~0ull;
__device__ __forceinline__ unsigned long long mix64(unsigned long long x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
	return x;
}
// (hm: mix64(key), for a caller that has it already)
__device__ __forceinline__ void hash_insert_mixed(unsigned long long* tab, unsigned long long mask, unsigned long long key, unsigned long long hm, int* overflow)
{
	unsigned long long h = hm & mask;
	for (int probe = 0; probe < 4096; probe++)
	{
		unsigned long long cur = tab[h];
		if (cur == key) return;
		if (cur == HEMPTY)
		{
			unsigned long long old = atomicCAS(&tab[h], HEMPTY, key);
			if (old == HEMPTY || old == key) return;
		}
		h = (h + 1) & mask;
	}
	*overflow = 1;
}
__device__ __forceinline__ void hash_insert(unsigned long long* tab, unsigned long long mask, unsigned long long key, int* overflow)
{
	hash_insert_mixed(tab, mask, key, mix64(key), overflow);
}
// A work-group's own set (LDS, open addressing) of the keys it has already sent to the table.  Neighbouring features are seen by the
// same poses, so nearly every pair a work-group forms it has formed before: only a key NEW to the work-group goes to the global table.
// A key that finds neither itself nor a free slot within PAIRSET_PROBES steps -- the set is full around it -- goes to the global table
// directly: the result is a set union, so that is always correct.  (The lane that put a key into the set is the one that inserts it:
// every key of the set is in the table when the kernel ends.)
constexpr int PAIRSET_SLOTS = 2048; // 16 KB of LDS
constexpr int PAIRSET_PROBES = 8;
__device__ __forceinline__ void pairset_clear(unsigned long long* set) // (the caller synchronises the work-group)
{
	for (int i = threadIdx.x; i < PAIRSET_SLOTS; i += blockDim.x) set[i] = HEMPTY;
}
__device__ __forceinline__ void pairset_insert(unsigned long long* set, unsigned long long* tab, unsigned long long mask, unsigned long long key, int* overflow)
{
	const unsigned long long hm = mix64(key);
	unsigned s = (unsigned)(hm >> 40) & (PAIRSET_SLOTS - 1);
	for (int probe = 0; probe < PAIRSET_PROBES; probe++)
	{
		unsigned long long cur = set[s];
		if (cur == HEMPTY) cur = atomicCAS(&set[s], HEMPTY, key); // HEMPTY: this lane has put it there
		if (cur == key) return;
		if (cur == HEMPTY) break;
		s = (s + 1) & (PAIRSET_SLOTS - 1);
	}
	hash_insert_mixed(tab, mask, key, hm, overflow);
}
__device__ __forceinline__ int hash_find(const unsigned long long* __restrict__ tab, const int* __restrict__ val, unsigned long long mask,
                                         unsigned long long key)
{
	unsigned long long h = mix64(key) & mask;
	for (int probe = 0; probe < 4096; probe++)
	{
		unsigned long long cur = tab[h];
		if (cur == key) return val[h];
		if (cur == HEMPTY) return -1;
		h = (h + 1) & mask;
	}
	return -1;
}
__device__ __forceinline__ unsigned long long pair_key(int p, int q)
{
	return p <= q ? (((unsigned long long)(unsigned)p << 32) | (unsigned)q) : (((unsigned long long)(unsigned)q << 32) | (unsigned)p);
}

} // namespace lsfm
