// K8: the block pattern of the camera system S = U - W V^-1 W^T of a level -- a hash set of the pose pairs that share a feature plus
// U's pattern (replaces the dense byte mask smask, Imp.cpp:2131-2205), compacted and sorted into block CSR.  It depends on index
// arrays only, so it can be made from more than one place:
//   build_schur_pattern           from the joint map (pat_insert_w); a Mono level: seeded from the level below (PatternSeed); a
//                                 feature-sharded run: the union over the ranks
//   schur_pattern_early_*         earlier, from the inputs of a Stereo level, while its transform runs
//   schur_pattern_prefetch        one level ahead, from this level's joint maps, with what the next level's transform and join count
// All of them are the same steps (PatternBuild): table set-up, [inserts], compaction (all enqueued); then -- after the one read-back of
// the count -- sort, block CSR and the SpMV index (build_spmv_index, lsfm_solve.hip).  schur_pattern_check compares a pattern made
// ahead with the joint map's.
#include <algorithm>

#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_join.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

// ---- the inserts ----------------------------------------------------------------------------------------------------------------
__global__ void k_fill_u64(unsigned long long* p, size_t n, unsigned long long v)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = v;
}

__global__ void k_pat_insert_keys(int n, const unsigned long long* __restrict__ keys, unsigned long long* tab, unsigned long long mask, int* overflow)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) hash_insert(tab, mask, keys[i], overflow);
}

// U's pairs and every block row's diagonal block.  pose_map / hub (optional, made ahead of the transform): + the link of every pose to
// the hub pose of its map -- U' holds (k, hub) for every pose k of a transformed map (Imp.cpp:711-723); hub < 0: passed through
__global__ void k_pat_insert_u(int NU, int M, const int* __restrict__ Ui, const int* __restrict__ Uj, const int* __restrict__ pose_map,
                               const int* __restrict__ hub, unsigned long long* tab, unsigned long long mask, int* overflow)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < NU) hash_insert(tab, mask, pair_key(Ui[i], Uj[i]), overflow);
	if (i < M)
	{
		hash_insert(tab, mask, pair_key(i, i), overflow);
		const int h = hub ? hub[pose_map[i]] : -1;
		if (h >= 0) hash_insert(tab, mask, pair_key(i, h), overflow);
	}
}

// the pattern of the level below through the join's pose renumbering (PatternSeed)
__global__ void k_pat_insert_keys_remap(int n, const unsigned long long* __restrict__ keys, const int* __restrict__ pnew, const unsigned char* __restrict__ dropped,
                                        unsigned long long* tab, unsigned long long mask, int* overflow)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int a = (int)(keys[i] >> 32), b = (int)(keys[i] & 0xffffffffull);
	if (dropped[a] || dropped[b]) return;
	hash_insert(tab, mask, pair_key(pnew[a], pnew[b]), overflow);
}
// ---- pose pairs of features -------------------------------------------------------------------------------------------------------
// A feature is seen by the poses of up to two W runs (E: photo[jE .. jE + lenE), C likewise), each with the hub pose of its map behind it
// where the map is transformed on the way (hE / hC >= 0).  ALL: every pair of that list; CROSS: every pair of an E pose with a C pose.
// How the runs of feature f are found:
//   the joint map itself (pat_insert_w, Imp.cpp:2155-2173)        E = f, no C                                        ALL
//   the inputs of a Stereo level (schur_pattern_early_issue)      E = srcE[f], C = srcC[f], either may be missing, hubs ALL
//     The joint map of a Stereo join is the two input maps side by side: a joint feature is seen by the poses of its End source,
//     the poses of its Cur source, and the hub pose of either map that is transformed on the way (the transform gives every feature
//     of the map a block to the hub pose, Imp.cpp:1303-1309, and folds old blocks to it into that one).  All of that is known from the
//     level's INPUT index arrays once the features are matched -- before the transform's block kernels have run.
//   one level ahead (schur_pattern_prefetch)                      C = f (second map of a pair), E = match[f], hubs   CROSS
//   a Mono level seeded from the level below (PatternSeed)        E = srcE[f], C = srcC[f], poses renumbered by the join (pnew, dropped)  CROSS
// The two CROSS callers first make the features that have both runs dense (k_pat_dense_matched: `list`, `count` on the device), so
// that no work-group is mostly idle lanes.
// A work-group of PAT_WG lanes takes PAT_RUN consecutive features of the (dense) list at a time and spreads ALL their pairs over its
// lanes (a prefix sum of the pair counts; a lane finds its feature by bisection), so long and short runs fill the lanes alike; the
// pairs go through the work-group's own set (pairset_insert, lsfm_solve.hpp), which is emptied for every run of features.
constexpr int PAT_RUN = 32;
constexpr int PAT_WG = 256;
struct PatFeat { int jE, lenE, hE, jC, lenC, hC; };
struct PatPairsIn {
	int n = 0;                                    // features (an upper bound where count is given)
	const int *count = nullptr, *list = nullptr;  // the dense list and its length on the device; null: the features 0 .. n-1
	const int *srcE = nullptr, *srcC = nullptr, *match = nullptr;
	const int *fptr = nullptr, *photo = nullptr;
	const int *feat_map = nullptr, *hub = nullptr; // hub pose of the map of a feature; null: none
	const int* pnew = nullptr;                     // renumbering of the poses; null: none
	const unsigned char* dropped = nullptr;
};
template <bool CROSS>
__global__ void __launch_bounds__(PAT_WG)
k_pat_insert_pairs(PatPairsIn in, unsigned long long* tab, unsigned long long mask, int* overflow)
{
	__shared__ unsigned long long set[PAIRSET_SLOTS];
	__shared__ PatFeat feats[PAT_RUN];
	__shared__ unsigned long long pre[PAT_RUN + 1]; // pre[i]: pairs of the features before i of this run
	static_assert(PAT_RUN <= LSFM_WAVE && (PAT_RUN & (PAT_RUN - 1)) == 0, "one wave loads a run of features");
	const int n = in.count ? min(*in.count, in.n) : in.n;
	const int tid = threadIdx.x;
	for (int r0 = blockIdx.x * PAT_RUN; r0 < n; r0 += gridDim.x * PAT_RUN)
	{
		pairset_clear(set);
		if (tid < LSFM_WAVE)
		{
			PatFeat f = { 0, 0, -1, 0, 0, -1 };
			unsigned long long np = 0;
			if (tid < PAT_RUN && r0 + tid < n)
			{
				const int x = in.list ? in.list[r0 + tid] : r0 + tid;
				const int fe = in.srcE ? in.srcE[x] : (in.match ? in.match[x] : x);
				const int fc = in.srcC ? in.srcC[x] : (in.match ? x : -1);
				if (fe >= 0) { f.jE = in.fptr[fe]; f.lenE = in.fptr[fe + 1] - f.jE; if (in.hub) f.hE = in.hub[in.feat_map[fe]]; }
				if (fc >= 0) { f.jC = in.fptr[fc]; f.lenC = in.fptr[fc + 1] - f.jC; if (in.hub) f.hC = in.hub[in.feat_map[fc]]; }
				const unsigned long long LE = f.lenE + (f.hE >= 0 ? 1 : 0), LC = f.lenC + (f.hC >= 0 ? 1 : 0);
				// ALL: pair (a, a + d) of the list taken as a ring, d = 1 .. L / 2 -- every pair once (twice at d = L / 2 of an even L)
				np = CROSS ? LE * LC : (LE + LC) * ((LE + LC) / 2);
			}
			unsigned long long sum = np;
#pragma unroll
			for (int off = 1; off < PAT_RUN; off <<= 1)
			{
				const unsigned long long v = (unsigned long long)__shfl_up((long long)sum, off, LSFM_WAVE);
				if (tid >= off) sum += v;
			}
			if (tid < PAT_RUN) { feats[tid] = f; pre[tid + 1] = sum; }
			if (tid == 0) pre[0] = 0;
		}
		__syncthreads();
		const unsigned long long P = pre[PAT_RUN];
		for (unsigned long long g = tid; g < P; g += PAT_WG)
		{
			int lo = 0, hi = PAT_RUN; // pre[lo] <= g < pre[hi]
			while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pre[mid] <= g) lo = mid; else hi = mid; }
			const PatFeat f = feats[lo];
			const unsigned idx = (unsigned)(g - pre[lo]);
			const int LE = f.lenE + (f.hE >= 0 ? 1 : 0), LC = f.lenC + (f.hC >= 0 ? 1 : 0);
			int a, b;
			if (CROSS) { a = (int)(idx / (unsigned)LC); b = LE + (int)(idx - (unsigned)a * (unsigned)LC); }
			else
			{
				const int L = LE + LC, half = L / 2;
				a = (int)(idx / (unsigned)half);
				b = a + 1 + (int)(idx - (unsigned)a * (unsigned)half);
				if (b >= L) b -= L;
			}
			auto pose_at = [&](int i) -> int {
				int p;
				if (i < LE) p = i < f.lenE ? in.photo[f.jE + i] : f.hE;
				else { i -= LE; p = i < f.lenC ? in.photo[f.jC + i] : f.hC; }
				if (in.pnew) p = in.dropped[p] ? -1 : in.pnew[p];
				return p;
			};
			const int pa = pose_at(a), pb = pose_at(b);
			if (pa >= 0 && pb >= 0) pairset_insert(set, tab, mask, pair_key(pa, pb), overflow);
		}
		__syncthreads(); // (the next run overwrites feats, pre and the set)
	}
}
template <bool CROSS>
static void pat_insert_pairs(hipStream_t s, const PatPairsIn& in, unsigned long long* tab, unsigned long long mask, int* overflow)
{
	if (in.n <= 0) return;
	const unsigned grid = (unsigned)std::min(2048, (in.n + PAT_RUN - 1) / PAT_RUN);
	hipLaunchKernelGGL(k_pat_insert_pairs<CROSS>, dim3(grid), dim3(PAT_WG), 0, s, in, tab, mask, overflow);
}

// the slot of every lane that has something to append to a list whose length is *count: one atomic per work-group (256 lanes, all call)
__device__ __forceinline__ int wg_append_slot(bool have, int* count)
{
	__shared__ int wave_n[256 / LSFM_WAVE], base;
	const unsigned long long m = __ballot(have);
	const int lane = threadIdx.x & (LSFM_WAVE - 1), w = threadIdx.x / LSFM_WAVE;
	if (lane == 0) wave_n[w] = __popcll(m);
	__syncthreads();
	if (threadIdx.x == 0)
	{
		int total = 0;
		for (int k = 0; k < 256 / LSFM_WAVE; k++) total += wave_n[k];
		base = total ? atomicAdd(count, total) : 0;
	}
	__syncthreads();
	int slot = base + __popcll(m & ((1ull << lane) - 1ull));
	for (int k = 0; k < w; k++) slot += wave_n[k];
	return slot;
}
// the features that have both runs (a[i] >= 0, b[i] >= 0 where given), of the second map of a pair (odd_of[i] odd, where given)
__global__ void __launch_bounds__(256)
k_pat_dense_matched(int n, const int* __restrict__ a, const int* __restrict__ b, const int* __restrict__ odd_of, int* __restrict__ list, int* __restrict__ count)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool have = i < n && a[i] >= 0 && (!b || b[i] >= 0) && (!odd_of || (odd_of[i] & 1));
	const int slot = wg_append_slot(have, count);
	if (have) list[slot] = i;
}

// ---- table -> sorted key list -> block CSR ----------------------------------------------------------------------------------------
// (the order of `list` is free -- it is sorted next --, the count exact)
__global__ void __launch_bounds__(256)
k_pat_compact(size_t cap, const unsigned long long* __restrict__ tab, unsigned long long* __restrict__ list, int* __restrict__ count)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long k = i < cap ? tab[i] : HEMPTY;
	const int slot = wg_append_slot(k != HEMPTY, count);
	if (k != HEMPTY) list[slot] = k;
}

// (row << 32 | column) -> (row << rb | column), both below 2^rb: the bits the sort has to look at, next to each other
__global__ void k_pat_pack(int n, unsigned long long* __restrict__ keys, int rb)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = ((keys[i] >> 32) << rb) | (keys[i] & 0xffffffffull);
}
// packed: the sorted packed keys; sorted: the same as (row << 32 | column)
__global__ void k_pat_assign(int nnzb, const unsigned long long* __restrict__ packed, int rb, unsigned long long* __restrict__ sorted,
                             const unsigned long long* __restrict__ tab, int* __restrict__ val, unsigned long long mask, int* __restrict__ colidx)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nnzb) return;
	const unsigned long long pk = packed[i];
	const unsigned long long key = ((pk >> rb) << 32) | (pk & ((1ull << rb) - 1ull));
	sorted[i] = key;
	unsigned long long h = mix64(key) & mask;
	while (tab[h] != key) h = (h + 1) & mask;
	val[h] = i;
	colidx[i] = (int)(key & 0xffffffffull);
}

// rowptr[r] = first index whose key >= (r << 32)
__global__ void k_rowptr_from_keys(int rows, int n, const unsigned long long* __restrict__ sorted, int shift, int* __restrict__ rowptr)
{
	int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > rows) return;
	unsigned long long target = (unsigned long long)(unsigned)r << shift;
	int lo = 0, hi = n;
	while (lo < hi) { int mid = (lo + hi) >> 1; if (sorted[mid] < target) lo = mid + 1; else hi = mid; }
	rowptr[r] = lo;
}
void rowptr_from_keys(lsfm_context* ctx, int M, int cnt, const unsigned long long* sorted_upper, int* rowptr)
{
	hipLaunchKernelGGL(k_rowptr_from_keys, dim3((M + 1 + 255) / 256), dim3(256), 0, ctx->stream, M, cnt, sorted_upper, 32, rowptr);
}

struct PatternBuild {
	unsigned long long *tab = nullptr, *list = nullptr;
	int *hval = nullptr, *d_flags = nullptr; // [0] overflow, [1] count, [2] length of the dense feature list of the cross pairs
	size_t cap = 0;
	unsigned long long mask() const { return (unsigned long long)(cap - 1); }
};
static size_t pattern_capacity(size_t NU, size_t M)
{
	// S has little more than U's pattern (the W-induced pairs are mostly hub links that U already holds): 4x head room over
	// NU + 8 M entries; a table that overflows is rebuilt larger
	size_t cap = 1024;
	while (cap < 4 * (NU + 8 * M + 64)) cap <<= 1;
	return cap;
}
static void pattern_begin(lsfm_context* ctx, size_t cap, PatternBuild& pb)
{
	Arena& sc = ctx->scratch;
	pb.cap = cap;
	pb.tab = sc.alloc<unsigned long long>(cap);
	pb.hval = sc.alloc<int>(cap);
	pb.list = sc.alloc<unsigned long long>(cap);
	pb.d_flags = sc.alloc<int>(4);
	dev_zero(ctx, pb.d_flags, 4 * sizeof(int));
	hipLaunchKernelGGL(k_fill_u64, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, ctx->stream, pb.tab, cap, HEMPTY);
}
// all pose pairs of every feature's W run
static void pat_insert_w(hipStream_t s, int NF, const int* fptr, const int* photo, const PatternBuild& pb)
{
	PatPairsIn in;
	in.n = NF; in.fptr = fptr; in.photo = photo;
	pat_insert_pairs<false>(s, in, pb.tab, pb.mask(), pb.d_flags);
}
// the cross pairs of the features that have both runs (k_pat_dense_matched), on ctx->stream; once per table
static void pat_insert_matched_pairs(lsfm_context* ctx, PatPairsIn in, const int* a, const int* b, const int* odd_of, const PatternBuild& pb)
{
	int* dense = ctx->scratch.alloc<int>(in.n);
	hipLaunchKernelGGL(k_pat_dense_matched, dim3((in.n + 255) / 256), dim3(256), 0, ctx->stream, in.n, a, b, odd_of, dense, pb.d_flags + 2);
	in.list = dense; in.count = pb.d_flags + 2;
	pat_insert_pairs<true>(ctx->stream, in, pb.tab, pb.mask(), pb.d_flags);
}
static void pattern_compact(lsfm_context* ctx, PatternBuild& pb)
{
	hipLaunchKernelGGL(k_pat_compact, dim3((unsigned)((pb.cap + 255) / 256)), dim3(256), 0, ctx->stream, pb.cap, pb.tab, pb.list, pb.d_flags + 1);
}
// reads the count back (synchronises ctx->stream); false: the table overflowed or is more than half full
static bool pattern_count(lsfm_context* ctx, const PatternBuild& pb, int* cnt)
{
	int fl[2];
	d2h_ints(ctx, pb.d_flags, fl, 2);
	*cnt = fl[1];
	return !fl[0] && (size_t)fl[1] * 2 <= pb.cap;
}
// Feature-sharded run: the pattern of S is the UNION of what the ranks' slices induce.  Every rank learns every rank's count (a
// vector with one slot per rank, summed), then every rank's keys (each writes its list at its offset of a zeroed array, summed as
// integers), inserts them all and compacts again.  A rank whose table overflowed (!ok) says so in the count exchange: the same
// answer on every rank, so all of them start over with a larger table together.
static bool pattern_union_over_ranks(lsfm_context* ctx, PatternBuild& pb, bool ok, int* cnt)
{
	hipStream_t s = ctx->stream;
	Comm& cm = *ctx->comm;
	cm.restart();
	long long* d_counts = cm.alloc<long long>(cm.world + 1);
	std::vector<long long> hc(cm.world + 1, 0);
	hc[cm.rank] = ok ? *cnt : 0;
	hc[cm.world] = ok ? 0 : 1;
	h2d(ctx, d_counts, hc.data(), sizeof(long long) * hc.size());
	cm.allreduce(s, d_counts, hc.size(), LSFM_DTYPE_I64);
	d2h(ctx, hc.data(), d_counts, sizeof(long long) * hc.size());
	if (hc[cm.world] != 0) return false;
	long long total = 0, mine = 0;
	for (int r = 0; r < cm.world; r++) { if (r == cm.rank) mine = total; total += hc[r]; }
	if ((size_t)total * 2 > pb.cap) return false;
	unsigned long long* all = cm.alloc<unsigned long long>((size_t)total + 1);
	fill_async(s, all, 0, sizeof(unsigned long long) * (size_t)total);
	if (*cnt) LSFM_CHECK_HIP(hipMemcpyAsync(all + mine, pb.list, sizeof(unsigned long long) * (size_t)*cnt, hipMemcpyDeviceToDevice, s));
	cm.allreduce(s, all, (size_t)total, LSFM_DTYPE_I64);
	if (total) hipLaunchKernelGGL(k_pat_insert_keys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (int)total, all, pb.tab, pb.mask(), pb.d_flags);
	dev_zero(ctx, pb.d_flags + 1, sizeof(int));
	pattern_compact(ctx, pb);
	return pattern_count(ctx, pb, cnt); // replicated from here on: the same table contents on every rank
}
// sorted key list + block CSR: all that the host's symbolic analysis and K9 wait for (enqueued, nothing read back)
static void pattern_finish(lsfm_context* ctx, int M, const PatternBuild& pb, int cnt, SchurSystem& sy)
{
	Arena& sc = ctx->scratch;
	sy.M = M;
	sy.nnzb = cnt;
	// keys are (row << 32 | column) with both below M < 2^rb: ONE sort, of the keys packed to (row << rb | column), over their 2 rb
	// bits, out of place; k_pat_assign unpacks them into the list again.  That is the one path for every size: a list of some 10^5
	// keys or fewer rocPRIM merge-sorts whatever the bit range (one block sort + a few merges; two sorts over rb bits each were two of
	// those and two runtime copies), a larger one it radix-sorts, and 2 rb bits in one sort are never more passes than rb bits twice.
	int rb = 1;
	while ((1 << rb) <= M) rb++;
	unsigned long long* packed = sc.alloc<unsigned long long>(cnt + 1);
	if (cnt) hipLaunchKernelGGL(k_pat_pack, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, cnt, pb.list, rb);
	dev_sort_keys_u64(ctx, pb.list, packed, cnt, 0, 2 * rb);
	sy.rowptr = sc.alloc<int>(M + 1);
	sy.colidx = sc.alloc<int>(cnt + 1);
	if (cnt) hipLaunchKernelGGL(k_pat_assign, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, cnt, packed, rb, pb.list, pb.tab, pb.hval, pb.mask(), sy.colidx);
	rowptr_from_keys(ctx, M, cnt, pb.list, sy.rowptr);
	sy.tab = pb.tab; sy.hval = pb.hval; sy.mask = pb.mask();
	sy.upper_keys = pb.list;
	LSFM_CHECK_HIP(hipGetLastError());
}
// The whole of it on ctx->stream: `inserts(pb)` enqueues the pair inserts into a table of `cap` slots; a table that overflowed is
// released and built again four times as large.  false: it kept overflowing.
template <class Inserts>
static bool pattern_build(lsfm_context* ctx, int M, size_t cap, SchurSystem& sy, Inserts inserts)
{
	Arena& sc = ctx->scratch;
	for (int attempt = 0; attempt < 12; attempt++, cap <<= 2)
	{
		const size_t mk = sc.mark();
		PatternBuild pb;
		pattern_begin(ctx, cap, pb);
		inserts(pb);
		pattern_compact(ctx, pb);
		int cnt = 0;
		bool ok = pattern_count(ctx, pb, &cnt);
		if (ctx->comm) ok = pattern_union_over_ranks(ctx, pb, ok, &cnt);
		if (ok)
		{
			pattern_finish(ctx, M, pb, cnt, sy);
			build_spmv_index(ctx, sy, pb.list);
			return true;
		}
		sc.release(mk);
	}
	return false;
}

// ---- from the joint map ---------------------------------------------------------------------------------------------------------------
void build_schur_pattern(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy)
{
	hipStream_t s = ctx->stream;
	const int M = io.M, NF = io.NF;
	const PatternSeed* sd = (io.seed && io.seed->prev_keys && !ctx->comm) ? io.seed : nullptr;
	const bool built = pattern_build(ctx, M, pattern_capacity(io.NU, M), sy, [&](const PatternBuild& pb) {
		const int nu = std::max(io.NU, M);
		if (nu) hipLaunchKernelGGL(k_pat_insert_u, dim3((nu + 255) / 256), dim3(256), 0, s, io.NU, M, io.Ui, io.Uj, (const int*)nullptr, (const int*)nullptr, pb.tab, pb.mask(), pb.d_flags);
		if (sd)
		{
			// (until round 5 every Mono level that analyses hashed every pose pair of every feature again: 66 GB and 28 ms of a
			// synth-16k tree, profiles/r04_pmc_traffic_summary_synth16k.json)
			if (sd->prev_nnzb) hipLaunchKernelGGL(k_pat_insert_keys_remap, dim3((sd->prev_nnzb + 255) / 256), dim3(256), 0, s, sd->prev_nnzb, sd->prev_keys, sd->pnew, sd->dropped, pb.tab, pb.mask(), pb.d_flags);
			// ... and the pairs across the two sources of a matched joint feature
			if (sd->NFY)
			{
				PatPairsIn in;
				in.n = sd->NFY; in.srcE = sd->srcE; in.srcC = sd->srcC; in.fptr = sd->fptr_in; in.photo = sd->photo_in; in.pnew = sd->pnew; in.dropped = sd->dropped;
				pat_insert_matched_pairs(ctx, in, sd->srcE, sd->srcC, nullptr, pb);
			}
		}
		else pat_insert_w(s, NF, io.fptr, io.photo, pb);
	});
	if (!built) LSFM_FAIL(LSFM_ERR_INTERNAL, "Schur pattern hash table kept overflowing");
	// debug / test: a pair the seeded pattern lacked would lose its share of S without a word
	if (sd && getenv("LSFM_CHECK_MONO_SEED")) schur_pattern_check(ctx, io, sy, "seeded");
}

void schur_pattern_only(lsfm_context* ctx, const SolveIO& io, int* nnzb, const int** rowptr, const int** colidx)
{
	SchurSystem sy;
	build_schur_pattern(ctx, io, sy);
	*nnzb = sy.nnzb; *rowptr = sy.rowptr; *colidx = sy.colidx;
}

void schur_pattern_check(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const char* what)
{
	LSFM_CHECK_HIP(hipDeviceSynchronize());
	SolveIO plain = io;
	plain.seed = nullptr;
	SchurSystem ref;
	build_schur_pattern(ctx, plain, ref);
	std::vector<unsigned long long> a(sy.nnzb), b(ref.nnzb);
	d2h(ctx, a.data(), sy.upper_keys, a.size() * sizeof(unsigned long long));
	d2h(ctx, b.data(), ref.upper_keys, b.size() * sizeof(unsigned long long));
	if (a != b) LSFM_FAIL(LSFM_ERR_INTERNAL, std::string(what) + " pattern of S (" + std::to_string(a.size()) + " blocks) differs from the joint map's (" + std::to_string(b.size()) + ")");
}

// ---- earlier: from the inputs of a Stereo level, in two halves (no retry: an overflow falls back to build_schur_pattern) ----------------
struct EarlyPattern { PatternBuild pb; int M = 0; };

void schur_pattern_early_issue(lsfm_context* ctx, const EarlyPatternIn& in)
{
	ctx->early.reset();
	auto ep = std::make_shared<EarlyPattern>();
	ep->M = in.M;
	// on the side stream, behind the point of the main stream where the matches and the hub poses are known (the caller recorded
	// evC_pairs).  Rejoins with the second half, which follows it on that stream (level_structure, case 4)
	{
		Fork side(ctx, ctx->stream3, evC_pairs, false);
		hipStream_t s = ctx->stream;
		PatternBuild& pb = ep->pb;
		pattern_begin(ctx, pattern_capacity((size_t)in.NU + in.M, in.M), pb);
		const int nu = std::max(in.NU, in.M);
		if (nu) hipLaunchKernelGGL(k_pat_insert_u, dim3((nu + 255) / 256), dim3(256), 0, s, in.NU, in.M, in.Ui, in.Uj, in.pose_map, in.hub, pb.tab, pb.mask(), pb.d_flags);
		PatPairsIn pi;
		pi.n = in.NFY; pi.srcE = in.srcE; pi.srcC = in.srcC; pi.fptr = in.fptr; pi.photo = in.photo; pi.feat_map = in.feat_map; pi.hub = in.hub;
		pat_insert_pairs<false>(s, pi, pb.tab, pb.mask(), pb.d_flags);
		pattern_compact(ctx, pb);
		LSFM_CHECK_HIP(hipGetLastError());
	}
	ctx->early = ep;
}
void schur_pattern_early_drop(lsfm_context* ctx) { ctx->early.reset(); }

// Second half, on the stream ctx->stream currently names (the caller has swapped the side stream in): count, sort, block CSR.
// false: no early build in flight, or its table overflowed -- the caller builds the pattern from the joint map instead.
bool schur_pattern_early_finish(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy)
{
	std::shared_ptr<EarlyPattern> ep = std::move(ctx->early);
	if (!ep || ep->M != io.M) return false;
	int cnt = 0;
	if (!pattern_count(ctx, ep->pb, &cnt)) return false;
	pattern_finish(ctx, io.M, ep->pb, cnt, sy);
	return true;
}
// after the keys have gone to the host: -- enqueued only -- the SpMV index, which nothing needs before the first product of the CG
void schur_pattern_early_extras(lsfm_context* ctx, SchurSystem& sy) { build_spmv_index(ctx, sy, sy.upper_keys); }

// ---- one level ahead: the pattern of the NEXT level's system, from this level's joint maps (prefetch_next_level, lsfm_level.hip) -------
// hub pose of every map of the batch in the next level's transform
__global__ void k_pre_hubs(int M, const int* __restrict__ pose_id, const int* __restrict__ pose_map, const int* __restrict__ tref, int* __restrict__ hub)
{
	int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= M) return;
	const int b = pose_map[k];
	if (tr_stereo_hub(pose_id[k], tref[b])) hub[b] = k;
}
// which blocks of the batch survive the next level's transform as they are (what k_tr_flags of lsfm_transform.hip will find)
__global__ void k_pre_flags(const int* __restrict__ Ui, const int* __restrict__ Uj, int NU, const int* __restrict__ photo, int NW,
                            const int* __restrict__ pose_map, const int* __restrict__ hub, int* __restrict__ keepU, int* __restrict__ keepW)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < NU) keepU[i] = tr_keeps_u(Ui[i], Uj[i], hub[pose_map[Ui[i]]], -1);
	if (i < NW) keepW[i] = tr_keeps_w(photo[i], hub[pose_map[photo[i]]], -1);
	if (i == 0) { keepU[NU] = 0; keepW[NW] = 0; }
}
__global__ void k_pre_gather(const int* __restrict__ KU, const int* __restrict__ KW, const int* __restrict__ R, const int* __restrict__ uoff,
                             const int* __restrict__ woff, const int* __restrict__ foff, int B, int* __restrict__ out)
{
	int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b > B) return;
	out[b] = KU[uoff[b]];
	out[B + 1 + b] = KW[woff[b]];
	out[2 * (B + 1) + b] = R[foff[b]];
}
// ctx->stream / ctx->scratch name the stream and the arena the caller wants this on.  prev_keys: the pattern of the level that
// produced Y (every pair inside one of Y's maps).  false: nothing to build from.  counts (optional): what the next level's
// transform and join read back from the device -- kept-block prefixes at the map boundaries (U, then W: transform_batch's
// `cnt`) and the ranks of the unmatched features there (join_stereo_prepare's `rb`), 3 (B + 1) ints, valid after the
// caller's next synchronisation of the stream.
bool schur_pattern_prefetch(lsfm_context* ctx, const DevBatch& Y, const int* d_tref, const unsigned long long* prev_keys, int prev_nnzb, SchurSystem& sy,
                            std::vector<int>* counts, bool want_pattern, LevelIndex* keep)
{
	// prev_keys == null: the level that produced Y left no pattern (its systems were small enough for the dense path, which needs
	// none): the pairs inside every map of Y are then taken from Y's own W runs (pat_insert_w), as a level without a predecessor does
	if (!Y.M) return false;
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	int* hub = sc.alloc<int>(Y.B);
	fill_async(s, hub, 0xff, sizeof(int) * (size_t)Y.B);
	hipLaunchKernelGGL(k_pre_hubs, dim3((Y.M + 255) / 256), dim3(256), 0, s, Y.M, Y.pose_id, Y.pose_map, d_tref, hub);
	int* match = sc.alloc<int>(Y.NF + 1);
	int* unm = sc.alloc<int>(Y.NF + 2);
	if (Y.NF) join_match_features(ctx, Y, match, unm);
	else dev_zero(ctx, unm, 2 * sizeof(int));
	if (counts)
	{
		const int B = Y.B;
		int* keepU = sc.alloc<int>(Y.NU + 1); int* keepW = sc.alloc<int>(Y.NW + 1);
		int* KU = sc.alloc<int>(Y.NU + 2); int* KW = sc.alloc<int>(Y.NW + 2); int* R = sc.alloc<int>(Y.NF + 2);
		const int nmax = std::max(std::max(Y.NU, Y.NW), 1);
		hipLaunchKernelGGL(k_pre_flags, dim3((nmax + 255) / 256), dim3(256), 0, s, Y.Ui, Y.Uj, Y.NU, Y.photo, Y.NW, Y.pose_map, hub, keepU, keepW);
		dev_exclusive_scan(ctx, keepU, KU, Y.NU);
		dev_exclusive_scan(ctx, keepW, KW, Y.NW);
		dev_exclusive_scan(ctx, unm, R, Y.NF);
		int* d_off = sc.alloc<int>(2 * (B + 1));
		h2d(ctx, d_off, Y.u_off.data(), (B + 1) * sizeof(int));
		h2d(ctx, d_off + B + 1, Y.w_off.data(), (B + 1) * sizeof(int));
		int* d_cnt = sc.alloc<int>(3 * (B + 1));
		hipLaunchKernelGGL(k_pre_gather, dim3((B + 1 + 127) / 128), dim3(128), 0, s, KU, KW, R, d_off, d_off + B + 1, Y.d_feat_off, B, d_cnt);
		counts->resize(3 * (size_t)(B + 1));
		LSFM_CHECK_HIP(hipMemcpyAsync(counts->data(), d_cnt, counts->size() * sizeof(int), hipMemcpyDeviceToHost, s));
		if (keep)
		{
			// what the next level's transform and join would work out again from the same index arrays (they live in this arena until
			// the level after next prepares ITS successor)
			*keep = LevelIndex();
			keep->NU = Y.NU; keep->NW = Y.NW; keep->NF = Y.NF;
			keep->KU = KU; keep->KW = KW; keep->match = match; keep->R = R;
		}
	}
	if (!want_pattern)
	{
		// (the next level's systems are small: it needs the counts alone; they arrive with the caller's next synchronisation)
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		return true;
	}
	return pattern_build(ctx, Y.M, pattern_capacity(std::max((size_t)Y.NU + Y.M, (size_t)prev_nnzb + Y.M), Y.M), sy, [&](const PatternBuild& pb) {
		const int nu = std::max(Y.NU, Y.M);
		hipLaunchKernelGGL(k_pat_insert_u, dim3((nu + 255) / 256), dim3(256), 0, s, Y.NU, Y.M, Y.Ui, Y.Uj, Y.pose_map, hub, pb.tab, pb.mask(), pb.d_flags);
		if (prev_keys && prev_nnzb) hipLaunchKernelGGL(k_pat_insert_keys, dim3((prev_nnzb + 255) / 256), dim3(256), 0, s, prev_nnzb, prev_keys, pb.tab, pb.mask(), pb.d_flags);
		if (!prev_keys) pat_insert_w(s, Y.NF, Y.fptr, Y.photo, pb);
		// pairs across the two maps of a pair: the features of the second map that have a match in the first
		if (Y.NF)
		{
			PatPairsIn in;
			in.n = Y.NF; in.match = match; in.fptr = Y.fptr; in.photo = Y.photo; in.feat_map = Y.feat_map; in.hub = hub;
			pat_insert_matched_pairs(ctx, in, match, nullptr, Y.feat_map, pb);
		}
	});
}

} // namespace lsfm
