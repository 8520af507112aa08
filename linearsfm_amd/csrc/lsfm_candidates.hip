// Candidate feature pairs for the exact gate: a cell search with a sure bound (C ABI: lsfm_map_feature_pair_candidates; DESIGN.md
// section 19).  No reference counterpart.
//
// Every pair f < g of the map's features with |x_f - x_g|^2 <= radius^2 and, where the marginal blocks Sigma_ff are given,
//     q_fg = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d <= tau,     d = x_f - x_g.
// For any joint covariance Var(x_f - x_g) + Var(x_f + x_g) = 2 (Sigma_ff + Sigma_gg), so Var(x_f - x_g) <= 2 (Sigma_ff + Sigma_gg) and
// q_fg <= d^2_fg, the gate's own distance: a pair dropped here is one lsfm_map_feature_pair_gate would reject at tau.
//
// Pipeline: cell keys -> stable radix sort of (key, feature) -> the records in cell order + the table of occupied cells -> one wave per
// (cell, slice of 64 of its records) counts its pairs -> scan -> the same kernel fills -> sort by (f << 32) | g -> gather -> download.
//
// Cells.  Uniform grid, cell edge = radius (1 + 2^-20), NOT radius: with the edge equal to the radius two points exactly radius apart
// can land two cells apart once (x - lo) / edge has been rounded.  With the slack the quotients of two points within the radius differ
// by at most 1 - 2^-20 plus a rounding error of 2^-31 cells at most (21 bits of cell index, 52 of mantissa), so "within radius =>
// the same or a neighbouring cell" holds in floating point.  Cell index floor((x - lo) / edge) per axis, lo the bounding box's minimum,
// 21 bits per axis, key = ix << 42 | iy << 21 | iz.
//
// Half neighbourhood.  A pair is met once, from the cell with the smaller key: the cell itself and the 13 neighbours whose key offset
// is positive.  z is the lowest field of the key, so cells that differ in z alone are neighbours in the sorted order too, and those 14
// cells are 5 runs of consecutive records: {(0,0,0), (0,0,+1)}, {(0,+1,-1..+1)} and {(+1,dy,-1..+1)}, dy = -1, 0, +1.  Lanes 0..9 find
// the runs' ends by binary search in the cell table; the records of a run are streamed 64 at a time, one record per lane, and every
// lane walks the slice in LDS (all lanes read one address: a broadcast).  In the first run only sorted positions j > i are tested,
// which takes care of the slice's own cell.
//
// Reproducible: a wave emits in a fixed order (ballot + prefix count, no slot atomics), nothing is summed in floating point, and the
// final sort on the unique key fixes the order of the output whatever the kernels' own order is.
#include <climits>
#include <cmath>

#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"

namespace lsfm {

namespace {

constexpr int CAND_BITS = 21;                     // bits of a cell index per axis
constexpr long long CAND_MAXC = (1ll << CAND_BITS) - 1;
constexpr int CAND_WAVES = 4;                     // waves (= work items) of a work-group of the pair kernel
constexpr int CAND_RUNS = 5;                      // runs of consecutive records of a half neighbourhood

inline dim3 grid(size_t n, int block = 256) { return dim3((unsigned)std::max<size_t>(1, (n + block - 1) / block)); }

// key[i] of feature i and idx[i] = i
__global__ void __launch_bounds__(256) k_cand_keys(int n, const double* __restrict__ x, double lox, double loy, double loz, double edge,
                                                   unsigned long long* __restrict__ key, int* __restrict__ idx)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double lo[3] = { lox, loy, loz };
	unsigned long long k = 0;
#pragma unroll
	for (int a = 0; a < 3; a++)
	{
		long long c = (long long)floor((x[3 * (size_t)i + a] - lo[a]) / edge);
		c = c < 0 ? 0 : (c > CAND_MAXC ? CAND_MAXC : c); // (the host has checked the extent: a guard, not a rule)
		k = (k << CAND_BITS) | (unsigned long long)c;
	}
	key[i] = k;
	idx[i] = i;
}

// the records in cell order as planes rec[k][n]: k = 0..2 the coordinates, 3..8 the upper triangle of Sigma_ff row by row (COV); and
// head[p] = 1 where sorted position p opens a cell (head[n] = 0 for the scan)
template <bool COV>
__global__ void __launch_bounds__(256) k_cand_pack(int n, const unsigned long long* __restrict__ key, const int* __restrict__ idx, const double* __restrict__ x,
                                                   const double* __restrict__ cov, double* __restrict__ rec, int* __restrict__ head)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p > n) return;
	if (p == n) { head[n] = 0; return; }
	const int f = idx[p];
#pragma unroll
	for (int a = 0; a < 3; a++) rec[(size_t)a * n + p] = x[3 * (size_t)f + a];
	if (COV)
	{
		const double* c = cov + 9 * (size_t)f;
		rec[(size_t)3 * n + p] = c[0]; rec[(size_t)4 * n + p] = c[1]; rec[(size_t)5 * n + p] = c[2];
		rec[(size_t)6 * n + p] = c[4]; rec[(size_t)7 * n + p] = c[5]; rec[(size_t)8 * n + p] = c[8];
	}
	head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

// the table of occupied cells: ckey[c], cstart[c] (cstart[ncell] = n), from the scan of the heads
__global__ void __launch_bounds__(256) k_cand_cells(int n, const unsigned long long* __restrict__ key, const int* __restrict__ head, const int* __restrict__ rank,
                                                    unsigned long long* __restrict__ ckey, int* __restrict__ cstart)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	if (head[p]) { ckey[rank[p]] = key[p]; cstart[rank[p]] = p; }
	if (p == n - 1) cstart[rank[n]] = n;
}

// slices of 64 records per cell (nsl[ncell] = 0 for the scan), and the fullest cell
__global__ void __launch_bounds__(256) k_cand_slices(int ncell, const int* __restrict__ cstart, int* __restrict__ nsl, int* __restrict__ fullest)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c > ncell) return;
	if (c == ncell) { nsl[c] = 0; return; }
	const int cnt = cstart[c + 1] - cstart[c];
	nsl[c] = (cnt + LSFM_WAVE - 1) / LSFM_WAVE;
	atomicMax(fullest, cnt);
}

// item[t] = (cell, first sorted position) of work item t; a cell writes its own slices
__global__ void __launch_bounds__(256) k_cand_items(int ncell, const int* __restrict__ cstart, const int* __restrict__ sloff, int2* __restrict__ item)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= ncell) return;
	const int t0 = sloff[c], t1 = sloff[c + 1];
	for (int t = t0; t < t1; t++) item[t] = make_int2(c, cstart[c] + (t - t0) * LSFM_WAVE);
}

// first cell whose key is >= k (upper: > k), in [0, ncell]
__device__ __forceinline__ int cand_bound(const unsigned long long* __restrict__ ckey, int ncell, unsigned long long k, bool upper)
{
	int lo = 0, hi = ncell;
	while (lo < hi)
	{
		const int mid = (lo + hi) >> 1;
		const unsigned long long v = ckey[mid];
		if (upper ? v <= k : v < k) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// dx^2 + dy^2 + dz^2 summed left to right, every product and sum rounded on its own: the same bits whatever the compiler would contract
__device__ __forceinline__ double cand_dist2(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
	return (dx * dx + dy * dy) + dz * dz;
}

// q = 1/2 d^T M^-1 d by the LDL^T of M (upper triangle m00 m01 m02 m11 m12 m22) in registers; false: a pivot is not > 0 (NaN included)
__device__ __forceinline__ bool cand_q(const double* m, double dx, double dy, double dz, double& q)
{
	const double d0 = m[0];
	const double l10 = m[1] / d0, l20 = m[2] / d0;
	const double d1 = m[3] - l10 * m[1];
	const double t = m[4] - l20 * m[1];
	const double l21 = t / d1;
	const double d2 = m[5] - l20 * m[2] - l21 * t;
	const double y0 = dx, y1 = dy - l10 * y0, y2 = dz - l20 * y0 - l21 * y1;
	q = 0.5 * (y0 * y0 / d0 + y1 * y1 / d1 + y2 * y2 / d2);
	return d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}

// One wave per work item.  FILL = false: cnt[t] = pairs of item t (cnt[nitem] = 0 for the scan), and the sums of pair tests and pairs
// over all items (integer atomics, one per wave).  FILL = true: the pairs of item t at off[t] .. off[t + 1].
template <bool COV, bool FILL>
__global__ void __launch_bounds__(CAND_WAVES * LSFM_WAVE)
k_cand_pairs(int n, int ncell, int nitem, const int2* __restrict__ item, const unsigned long long* __restrict__ ckey, const int* __restrict__ cstart,
             const double* __restrict__ rec, const int* __restrict__ idx, double r2, double tau, int* __restrict__ cnt, unsigned long long* __restrict__ sums,
             const int* __restrict__ off, unsigned long long* __restrict__ okey, double* __restrict__ od2, double* __restrict__ oq)
{
	constexpr int NP = COV ? 9 : 3;
	__shared__ double srec[CAND_WAVES][NP][LSFM_WAVE];
	__shared__ int sidx[CAND_WAVES][LSFM_WAVE];
	const int lane = threadIdx.x & (LSFM_WAVE - 1), w = threadIdx.x / LSFM_WAVE;
	const int t = blockIdx.x * CAND_WAVES + w;
	const bool live = t < nitem;
	int cell = 0, s0 = 0, scnt = 0;
	if (live)
	{
		const int2 it = item[t];
		cell = it.x; s0 = it.y;
		scnt = min(LSFM_WAVE, cstart[cell + 1] - s0);
		if (lane < scnt)
		{
#pragma unroll
			for (int k = 0; k < NP; k++) srec[w][k][lane] = rec[(size_t)k * n + s0 + lane];
			sidx[w][lane] = idx[s0 + lane];
		}
	}
	__syncthreads(); // (the only one: from here on a wave reads its own part of the LDS)
	if (!live) { if (!FILL && t == nitem && lane == 0) cnt[nitem] = 0; return; }
	// ---- the ends of the 5 runs: lanes 2 r (first record) and 2 r + 1 (behind the last one) ----
	int pos = 0;
	if (lane == 0) pos = s0 + 1; // (the first run starts behind the slice's first record: only j > i is tested there)
	else if (lane < 2 * CAND_RUNS)
	{
		const unsigned long long k = ckey[cell];
		const long long ix = (long long)(k >> (2 * CAND_BITS)), iy = (long long)((k >> CAND_BITS) & CAND_MAXC), iz = (long long)(k & CAND_MAXC);
		const int r = lane >> 1;
		const bool upper = lane & 1;
		const long long cx = ix + (r >= 2 ? 1 : 0), cy = iy + (r == 1 ? 1 : (r >= 2 ? r - 3 : 0));
		const long long z0 = r == 0 ? iz : (iz > 0 ? iz - 1 : 0), z1 = iz < CAND_MAXC ? iz + 1 : CAND_MAXC;
		if (cx <= CAND_MAXC && cy >= 0 && cy <= CAND_MAXC)
		{
			const unsigned long long kk = ((unsigned long long)cx << (2 * CAND_BITS)) | ((unsigned long long)cy << CAND_BITS) | (unsigned long long)(upper ? z1 : z0);
			pos = cstart[cand_bound(ckey, ncell, kk, upper)];
		}
	}
	const unsigned long long below = (1ull << lane) - 1ull;
	int mine = 0;                 // FILL = false: this lane's pairs
	unsigned long long tests = 0; // ... and its pair tests
	int slot = FILL ? off[t] : 0;
	const int slot_end = FILL ? off[t + 1] : 0;
	for (int r = 0; r < CAND_RUNS; r++)
	{
		const int b = __shfl(pos, 2 * r, LSFM_WAVE), e = __shfl(pos, 2 * r + 1, LSFM_WAVE);
		for (int base = b; base < e; base += LSFM_WAVE)
		{
			const int j = base + lane;
			const bool act = j < e;
			double xj = 0.0, yj = 0.0, zj = 0.0, cj[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
			int g = 0;
			if (act)
			{
				xj = rec[j]; yj = rec[(size_t)n + j]; zj = rec[(size_t)2 * n + j];
				if (COV)
				{
#pragma unroll
					for (int k = 0; k < 6; k++) cj[k] = rec[(size_t)(3 + k) * n + j];
				}
				if (FILL) g = idx[j];
			}
			for (int i = 0; i < scnt; i++)
			{
				const bool ok = act && (r != 0 || j > s0 + i);
				const double dx = srec[w][0][i] - xj, dy = srec[w][1][i] - yj, dz = srec[w][2][i] - zj;
				const double d2 = cand_dist2(dx, dy, dz);
				bool pass = ok && d2 <= r2;
				double q = 0.0;
				if (COV && pass)
				{
					double m[6];
#pragma unroll
					for (int k = 0; k < 6; k++) m[k] = srec[w][3 + k][i] + cj[k];
					if (!cand_q(m, dx, dy, dz, q)) q = __longlong_as_double(0x7ff8000000000000ll); // kept: what cannot be bounded is not dropped
					else pass = q <= tau;
				}
				if (FILL)
				{
					const unsigned long long mask = __ballot(pass);
					if (mask)
					{
						const int at = slot + __popcll(mask & below);
						if (pass && at < slot_end)
						{
							const int f = sidx[w][i];
							okey[at] = ((unsigned long long)(unsigned)min(f, g) << 32) | (unsigned long long)(unsigned)max(f, g);
							od2[at] = d2;
							if (COV) oq[at] = q;
						}
						slot += __popcll(mask);
					}
				}
				else
				{
					mine += pass ? 1 : 0;
					tests += ok ? 1ull : 0ull;
				}
			}
		}
	}
	if (!FILL)
	{
		for (int o = LSFM_WAVE / 2; o; o >>= 1)
		{
			mine += __shfl_xor(mine, o, LSFM_WAVE);
			tests += (unsigned long long)__shfl_xor((long long)tests, o, LSFM_WAVE);
		}
		if (lane == 0)
		{
			cnt[t] = mine;
			atomicAdd(&sums[0], tests);
			atomicAdd(&sums[1], (unsigned long long)mine);
		}
	}
}

// the sorted pairs and their values: slot order -> (f, g) order
__global__ void __launch_bounds__(256) k_cand_gather(int total, const unsigned long long* __restrict__ key, const int* __restrict__ slot, const double* __restrict__ d2,
                                                     const double* __restrict__ q, int2* __restrict__ pairs, double* __restrict__ od2, double* __restrict__ oq)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= total) return;
	const unsigned long long v = key[k];
	pairs[k] = make_int2((int)(v >> 32), (int)(v & 0xffffffffull));
	const int s = slot[k];
	if (od2) od2[k] = d2[s];
	if (oq) oq[k] = q[s];
}

__global__ void __launch_bounds__(256) k_cand_iota(int total, int* __restrict__ v)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < total) v[k] = k;
}

int bits_of(unsigned long long v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

} // namespace

int map_feature_pair_candidates(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs, double* dist2, double* q,
                                long long cap, long long* count, double* times, long long* info)
{
	*count = 0;
	if (times) for (int k = 0; k < 4; k++) times[k] = 0.0;
	if (info) for (int k = 0; k < 4; k++) info[k] = 0;
	if (!std::isfinite(radius) || !(radius > 0.0)) LSFM_FAIL(LSFM_ERR_ARG, "radius must be finite and > 0");
	if (feat_cov && (!std::isfinite(tau) || !(tau > 0.0))) LSFM_FAIL(LSFM_ERR_ARG, "tau must be finite and > 0 when feat_cov is given");
	if (q && !feat_cov) LSFM_FAIL(LSFM_ERR_ARG, "q is asked for without feat_cov");
	const bool sizing = !pairs && cap == 0;
	if (!sizing && (!pairs || cap < 0)) LSFM_FAIL(LSFM_ERR_ARG, "pairs is null but cap is not 0");
	const int n = map->n;
	const double* x = map->stVal + (size_t)6 * map->m;
	double lo[3] = { 0.0, 0.0, 0.0 }, hi[3] = { 0.0, 0.0, 0.0 };
	for (int f = 0; f < n; f++)
		for (int a = 0; a < 3; a++)
		{
			const double v = x[3 * (size_t)f + a];
			if (!std::isfinite(v)) LSFM_FAIL(LSFM_ERR_ARG, "feature " + std::to_string(f) + " has a coordinate that is not finite");
			if (f == 0 || v < lo[a]) lo[a] = v;
			if (f == 0 || v > hi[a]) hi[a] = v;
		}
	if (n < 2) return LSFM_OK;
	if ((long long)n > (1ll << 25)) LSFM_FAIL(LSFM_ERR_ARG, "more than 2^25 features");
	const double edge = radius * (1.0 + std::ldexp(1.0, -20)); // NOT radius: see the head of this file
	unsigned long long cells_max = 0;
	for (int a = 0; a < 3; a++)
	{
		const double c = std::floor((hi[a] - lo[a]) / edge);
		if (!(c < (double)(1ll << CAND_BITS))) LSFM_FAIL(LSFM_ERR_ARG, "radius too small for the map's extent: more than 2^21 cells along an axis");
		if (a == 0) cells_max = (unsigned long long)c;
	}
	const int key_bits = std::max(1, 2 * CAND_BITS + bits_of(cells_max));
	const double r2 = radius * radius;
	const bool cov = feat_cov != nullptr;
	const int NP = cov ? 9 : 3;
	hipStream_t s = ctx->stream;
	hipEvent_t ev[5]; // start | keys | sorted, packed, cells and items known | counted and scanned | downloaded
	for (int k = 0; k < 5; k++) ev[k] = ctx->pool_event();
	size_t need = (size_t)n * 320 + ((size_t)64 << 20);
	for (int attempt = 0;; attempt++)
	{
		ctx->ensure_arenas(need);
		ctx->arena[0].reset(); ctx->scratch.reset();
		Arena& ar = ctx->arena[0];
		LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
		// ---- 1. upload, cell keys ----
		double* dx = ar.alloc<double>((size_t)3 * n);
		double* dcov = cov ? ar.alloc<double>((size_t)9 * n) : nullptr;
		h2d(ctx, dx, x, (size_t)3 * n * sizeof(double));
		if (cov) h2d(ctx, dcov, feat_cov, (size_t)9 * n * sizeof(double));
		unsigned long long* key = ar.alloc<unsigned long long>(n);
		int* idx = ar.alloc<int>(n);
		hipLaunchKernelGGL(k_cand_keys, grid(n), dim3(256), 0, s, n, dx, lo[0], lo[1], lo[2], edge, key, idx);
		LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
		// ---- 2. sort, records in cell order, the cell table, the work items ----
		dev_sort_pairs_u64(ctx, key, idx, n, key_bits);
		double* rec = ar.alloc<double>((size_t)NP * n);
		int* head = ar.alloc<int>((size_t)n + 1);
		int* rank = ar.alloc<int>((size_t)n + 1);
		if (cov) hipLaunchKernelGGL(k_cand_pack<true>, grid((size_t)n + 1), dim3(256), 0, s, n, key, idx, dx, dcov, rec, head);
		else hipLaunchKernelGGL(k_cand_pack<false>, grid((size_t)n + 1), dim3(256), 0, s, n, key, idx, dx, dcov, rec, head);
		dev_exclusive_scan(ctx, head, rank, n);
		const int ncell = d2h_int(ctx, rank + n);
		if (ncell < 1 || ncell > n) LSFM_FAIL(LSFM_ERR_INTERNAL, "the cell table has " + std::to_string(ncell) + " cells for " + std::to_string(n) + " features");
		unsigned long long* ckey = ar.alloc<unsigned long long>(ncell);
		int* cstart = ar.alloc<int>((size_t)ncell + 1);
		int* nsl = ar.alloc<int>((size_t)ncell + 1);
		int* sloff = ar.alloc<int>((size_t)ncell + 1);
		unsigned long long* sums = ar.alloc<unsigned long long>(4); // pair tests | pairs | fullest cell (int) | -
		dev_zero(ctx, sums, 4 * sizeof(unsigned long long));
		hipLaunchKernelGGL(k_cand_cells, grid(n), dim3(256), 0, s, n, key, head, rank, ckey, cstart);
		hipLaunchKernelGGL(k_cand_slices, grid((size_t)ncell + 1), dim3(256), 0, s, ncell, cstart, nsl, reinterpret_cast<int*>(sums + 2));
		dev_exclusive_scan(ctx, nsl, sloff, ncell);
		const int nitem = d2h_int(ctx, sloff + ncell);
		if (nitem < ncell || nitem > n) LSFM_FAIL(LSFM_ERR_INTERNAL, "the cells have " + std::to_string(nitem) + " slices for " + std::to_string(n) + " features");
		int2* item = ar.alloc<int2>(nitem);
		hipLaunchKernelGGL(k_cand_items, grid(ncell), dim3(256), 0, s, ncell, cstart, sloff, item);
		LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
		// ---- 3. count, scan ----
		int* cnt = ar.alloc<int>((size_t)nitem + 1);
		int* off = ar.alloc<int>((size_t)nitem + 1);
		const dim3 pg((unsigned)((size_t)nitem / CAND_WAVES + 1)); // (one wave more than items at least: it ends the scan's input)
		auto pass = [&](bool fill, unsigned long long* okey, double* od2, double* oq) {
			const dim3 blk(CAND_WAVES * LSFM_WAVE);
#define CAND_LAUNCH(C, F) hipLaunchKernelGGL((k_cand_pairs<C, F>), pg, blk, 0, s, n, ncell, nitem, item, ckey, cstart, rec, idx, r2, tau, cnt, sums, off, okey, od2, oq)
			if (cov) { if (fill) CAND_LAUNCH(true, true); else CAND_LAUNCH(true, false); }
			else { if (fill) CAND_LAUNCH(false, true); else CAND_LAUNCH(false, false); }
#undef CAND_LAUNCH
			LSFM_CHECK_HIP(hipGetLastError());
		};
		pass(false, nullptr, nullptr, nullptr);
		unsigned long long hs[4] = { 0, 0, 0, 0 };
		d2h(ctx, hs, sums, sizeof hs);
		if (hs[1] > (unsigned long long)INT_MAX) LSFM_FAIL(LSFM_ERR_ARG, std::to_string(hs[1]) + " candidates, more than 2^31 - 1: reduce the radius");
		const int total = (int)hs[1];
		dev_exclusive_scan(ctx, cnt, off, nitem);
		LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
		*count = total;
		if (info) { info[0] = ncell; info[1] = (long long)(int)(hs[2] & 0xffffffffull); info[2] = (long long)hs[0]; info[3] = total; }
		const bool fill = !sizing && total > 0;
		if (!sizing && (long long)total > cap)
		{
			LSFM_CHECK_HIP(hipStreamSynchronize(s));
			LSFM_FAIL(LSFM_ERR_ARG, "cap " + std::to_string(cap) + " is too small for " + std::to_string(total) + " candidates");
		}
		// ---- 4. fill, sort by (f, g), gather, download ----
		if (fill)
		{
			// slot-ordered key / slot / dist2 / q, the gathered pairs / dist2 / q, and the sort's own copies in the scratch arena
			const size_t out_need = (size_t)total * 56 + 4096, sort_need = (size_t)total * 16 + ((size_t)32 << 20);
			if (attempt == 0 && (ar.cap - ar.off < out_need || ctx->scratch.cap < sort_need))
			{
				LSFM_CHECK_HIP(hipStreamSynchronize(s));
				need += out_need + sort_need;
				continue; // once more from the upload, in arenas that hold the output (a second failure is LSFM_ERR_OOM)
			}
			unsigned long long* okey = ar.alloc<unsigned long long>(total);
			int* oslot = ar.alloc<int>(total);
			double* od2 = ar.alloc<double>(total);
			double* oq = cov ? ar.alloc<double>(total) : nullptr;
			int2* gp = ar.alloc<int2>(total);
			double* gd2 = dist2 ? ar.alloc<double>(total) : nullptr;
			double* gq = q ? ar.alloc<double>(total) : nullptr;
			pass(true, okey, od2, oq);
			hipLaunchKernelGGL(k_cand_iota, grid(total), dim3(256), 0, s, total, oslot);
			dev_sort_pairs_u64(ctx, okey, oslot, total, 32 + bits_of((unsigned long long)n));
			hipLaunchKernelGGL(k_cand_gather, grid(total), dim3(256), 0, s, total, okey, oslot, od2, oq, gp, gd2, gq);
			LSFM_CHECK_HIP(hipGetLastError());
			d2h(ctx, pairs, gp, (size_t)total * sizeof(int2));
			if (dist2) d2h(ctx, dist2, gd2, (size_t)total * sizeof(double));
			if (q) d2h(ctx, q, gq, (size_t)total * sizeof(double));
		}
		LSFM_CHECK_HIP(hipEventRecord(ev[4], s));
		LSFM_CHECK_HIP(hipEventSynchronize(ev[4]));
		if (times) for (int k = 0; k < 4; k++) times[k] = event_ms(ev[k], ev[k + 1]);
		return LSFM_OK;
	}
}

} // namespace lsfm
