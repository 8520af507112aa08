// Marginalising poses out of a map on the device (C ABI: lsfm_map_marginalise_poses).  No reference counterpart.
//
// Stage A is lsfm_map_marginalise over the features that go with the dropped poses: U1, canonical, the kept W / V untouched.  Stage B,
// with D the dropped and K the kept poses:
//     U'_KK = U1_KK - U1_KD U1_DD^-1 U1_DK
// U1_DD is factored by the covariance calls' own front end (cov_front on the pose-only sub-map of D, in whatever order the symbolic
// analysis likes): A = D^-1/2 P U1_DD P^T D^-1/2 = L L^T.  The correction is then a product of a matrix with its own transpose,
//     U1_KD U1_DD^-1 U1_DK = Y^T Y,   Y = L^-1 D^-1/2 P U1_DK,
// from a FORWARD sweep alone.  The symmetric form inherits the Cauchy-Schwarz bound |T_ij| <= sqrt(T_ii T_jj) element by element, which
// the solve-then-multiply form U1_KD (U1_DD^-1 U1_DK) only has norm-wise (DESIGN.md section 15 has the figures).
//
// Only the boundary poses Bd (kept poses with a block into D) have a column in Y.  They go in chunks of CC_KC = 32 poses through the
// side-by-side sweeps of lsfm_covcols.hip: a chunk is a slab [6 |D|][R], R = 6 k_c, in elimination order; every chunk's slab stays
// resident, one behind the other.  Full chunks are 192 columns = 12 whole 16-column tiles, so the 16-column tiles of ALL boundary
// columns (global column G = 6 * position in Bd + scalar, tile G / 16) never straddle two chunks.
//   k_pm_rhs   the sparse blocks of U1 between D and the chunk, scaled and permuted, into the zeroed slab
//   k_pm_syrk  T = Y^T Y on v_mfma_f64_16x16x4_f64 for the tile pairs that hold an output pair; no atomics, a fixed order
//   k_pm_emit  U'_ij = U1_ij - T_ij on the output pattern
// Y is stored dense although a column is zero outside the components next to its pose, and the contraction walks all rows.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "lsfm_chol.hpp"
#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_marg.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

namespace {

#define PM_CW (6 * CC_KC) /* columns of a full chunk */
#define PM_WAVES 4        /* waves of a k_pm_syrk work-group: the contraction is dealt among them */
static_assert(PM_CW % 16 == 0, "a column tile must not straddle two chunks");

// one block of U1 between a dropped pose and a boundary pose of the chunk
struct PmRhs {
	int blk;  // block of U1
	int drow; // the dropped pose's position in D (block row of U1_DD before the permutation)
	int col;  // the boundary pose's position in the chunk
	int tr;   // 1: the canonical orientation (row <= column) has the kept pose as the row -- read transposed
};

// slab[6 pinv[drow] + r][6 col + c] = dscale * U1_{D,b}[r][c]: D^-1/2 P U1_{D,b}, lane per number, six consecutive lanes on six
// consecutive doubles.  The slab was zeroed; a (dropped, kept) pair has one block, so no cell is written twice.
__global__ void k_pm_rhs(int nent, const PmRhs* __restrict__ ent, const double* __restrict__ U1, const int* __restrict__ pinv, const double* __restrict__ dscale,
                         int R, double* __restrict__ slab)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)nent * 36) return;
	const int e = (int)(idx / 36), q = (int)(idx - (size_t)e * 36);
	const int r = q / 6, c = q - 6 * r;
	const PmRhs en = ent[e];
	const double* blk = U1 + (size_t)en.blk * 36;
	const size_t row = (size_t)pinv[en.drow] * 6 + r;
	slab[row * R + en.col * 6 + c] = (en.tr ? blk[c * 6 + r] : blk[r * 6 + c]) * dscale[row];
}

typedef double pm_v4d __attribute__((ext_vector_type(4)));

// T[w] = Y[:, tile a]^T Y[:, tile b] for the tile pair w = (a <= b) of the work list, 16 x 16 doubles row-major.  Lane l feeds
// A[row l & 15][k = l >> 4] = Y[k][16 a + (l & 15)] and B[k = l >> 4][col l & 15] = Y[k][16 b + (l & 15)]: a row's 16 consecutive
// columns are contiguous, both operands load coalesced, and for a == b they are the same registers.  The contraction runs over the
// slab's NR = 6 |D| rows in steps of 4, dealt round-robin among the PM_WAVES waves; the partial tiles meet in LDS and are added in the
// order of the waves.  Given Y the result is the same bits on every call, and a diagonal tile is exactly symmetric: C[i][j] and C[j][i]
// are the same products in the same order.  Columns past Rtot (the last tile) and rows past NR (the last step of an odd |D|) enter as 0.
__global__ void __launch_bounds__(PM_WAVES * LSFM_WAVE) k_pm_syrk(const int2* __restrict__ work, int NR, int Rtot, const double* __restrict__ Y, double* __restrict__ T)
{
	__shared__ double red[PM_WAVES][256];
	const int w = blockIdx.x;
	const int ta = work[w].x, tb = work[w].y;
	const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, kq = lane >> 4, cl = lane & 15;
	const bool same = ta == tb;
	// the 16 columns of a tile lie in one chunk; a lane past the last column reads the tile's first column and contributes 0
	const int ga = ta * 16 + cl, gb = tb * 16 + cl;
	const bool va = ga < Rtot, vb = gb < Rtot;
	const int cha = (ta * 16) / PM_CW, chb = (tb * 16) / PM_CW;
	const int Ra = min(PM_CW, Rtot - cha * PM_CW), Rb = min(PM_CW, Rtot - chb * PM_CW);
	const double* pa = Y + (size_t)cha * NR * PM_CW + ((va ? ga : ta * 16) - cha * PM_CW);
	const double* pb = Y + (size_t)chb * NR * PM_CW + ((vb ? gb : tb * 16) - chb * PM_CW);
	const int nfull = NR / 4;
	pm_v4d acc = { 0.0, 0.0, 0.0, 0.0 };
	int ks = wave;
	for (; ks + 3 * PM_WAVES < nfull; ks += 4 * PM_WAVES) // four steps' loads in flight
	{
		double a[4], b[4];
#pragma unroll
		for (int u = 0; u < 4; u++)
		{
			const size_t row = (size_t)(4 * (ks + u * PM_WAVES) + kq);
			a[u] = pa[row * Ra];
			b[u] = same ? a[u] : pb[row * Rb];
		}
#pragma unroll
		for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? a[u] : 0.0, vb ? b[u] : 0.0, acc, 0, 0, 0);
	}
	for (; ks < nfull; ks += PM_WAVES)
	{
		const size_t row = (size_t)(4 * ks + kq);
		double a = pa[row * Ra];
		a = va ? a : 0.0;
		double b = a;
		if (!same)
		{
			b = pb[row * Rb];
			b = vb ? b : 0.0;
		}
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
	}
	if ((NR & 3) && wave == nfull % PM_WAVES) // the K tail
	{
		const int row = 4 * nfull + kq;
		const bool in = row < NR;
		const size_t rr = in ? (size_t)row : 0;
		double a = pa[rr * Ra], b = pb[rr * Rb];
		a = (in && va) ? a : 0.0;
		b = (in && vb) ? b : 0.0;
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
	}
#pragma unroll
	for (int reg = 0; reg < 4; reg++) red[wave][reg * 64 + lane] = acc[reg];
	__syncthreads();
	// lane l of register reg holds C[row (l >> 4) + 4 reg][col l & 15]
	double sum = red[0][tid];
#pragma unroll
	for (int v = 1; v < PM_WAVES; v++) sum += red[v][tid];
	const int reg = tid >> 6;
	T[(size_t)w * 256 + (kq + 4 * reg) * 16 + cl] = sum;
}

// U'[e] = U1[src[e]] - T on the output pattern (0 where U1 has no block, nothing taken off where the pair is no fill pair: bi < 0), lane
// per number.  T_ij[r][c] sits in the tile pair ((6 bi + r) / 16, (6 bj + c) / 16), whose place in the work list the host has put into
// widx[e][row tile 0 / 1][column tile 0 / 1].  A diagonal block is written from its upper triangle on both sides: exactly symmetric.
__global__ void k_pm_emit(int nout, const int* __restrict__ oUi, const int* __restrict__ oUj, const int* __restrict__ src, const int* __restrict__ bi,
                          const int* __restrict__ bj, const int* __restrict__ widx, const double* __restrict__ U1, const double* __restrict__ T,
                          double* __restrict__ out)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)nout * 36) return;
	const int e = (int)(idx / 36), q = (int)(idx - (size_t)e * 36);
	int r = q / 6, c = q - 6 * r;
	if (oUi[e] == oUj[e] && r > c) { const int t = r; r = c; c = t; }
	const int sb = src[e], pi = bi[e], pj = bj[e];
	double v = sb >= 0 ? U1[(size_t)sb * 36 + r * 6 + c] : 0.0;
	if (pi >= 0)
	{
		const int gr = 6 * pi + r, gc = 6 * pj + c;
		const int wi = widx[(size_t)e * 4 + (gr / 16 - (6 * pi) / 16) * 2 + (gc / 16 - (6 * pj) / 16)];
		v -= T[(size_t)wi * 256 + (gr & 15) * 16 + (gc & 15)];
	}
	out[idx] = v;
}

inline unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
inline unsigned long long tile_key(int a, int b) { return ((unsigned long long)(unsigned)a << 32) | (unsigned)b; }

} // namespace

int map_marginalise_poses(lsfm_context* ctx, const lsfm_map* map, bool mono, const unsigned char* keep_pose, const unsigned char* drop_feat, lsfm_map* out,
                          double* times, int* info)
{
	const int m = map->m;
	if (times) for (int k = 0; k < 5; k++) times[k] = 0.0;
	if (info) for (int k = 0; k < 8; k++) info[k] = 0;
	// ---- rules (host, labels alone) ----
	std::vector<unsigned char> drop;
	{
		std::string why;
		if (pose_marg_flags(map, mono, keep_pose, drop_feat, drop, why) != LSFM_OK) throw Error{ LSFM_ERR_ARG, why };
		if (drop.empty()) drop.push_back(0); // (n = 0: a pointer for stage A to hold)
	}
	hipStream_t s = ctx->stream;
	hipEvent_t ev[4] = { ctx->pool_event(), ctx->pool_event(), ctx->pool_event(), ctx->pool_event() }; // start | stage A on the host | sweeps done | downloaded
	LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	// ---- stage A: the features go, through the host ----
	MapOut A;
	{
		const int rc = map_marginalise(ctx, map, drop.data(), &A.g, nullptr);
		if (rc != LSFM_OK) return rc;
	}
	const lsfm_map& a = A.g;
	LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	// ---- structure ----
	PoseMargStructure st;
	pose_marg_structure(m, a.nU, a.Ui, a.Uj, keep_pose, st);
	const int nD = (int)st.dlist.size(), nK = (int)st.klist.size(), nBd = (int)st.bd.size(), nout = (int)st.oUi.size();
	const int nchunk = (nBd + CC_KC - 1) / CC_KC;
	if (info) { info[0] = nD; info[1] = nBd; info[2] = st.ncomp; info[3] = nout; info[4] = nchunk; }
	if (nD == 0)
	{
		// nothing to eliminate: stage A's map is the result
		LSFM_CHECK_HIP(hipEventSynchronize(ev[1]));
		if (times) times[0] = event_ms(ev[0], ev[1]);
		for (int e = 0; e < a.nU; e++) // the diagonal blocks from their upper triangle, as k_pm_emit writes them
			if (a.Ui[e] == a.Uj[e])
				for (int r = 1; r < 6; r++)
					for (int c = 0; c < r; c++) A.g.U[(size_t)e * 36 + r * 6 + c] = a.U[(size_t)e * 36 + c * 6 + r];
		A.give(out);
		return LSFM_OK;
	}
	// the pose-only sub-map of D (no gauge scalar is in D: mono = false)
	std::vector<int> sUi, sUj, sorg;
	std::vector<double> sU;
	std::vector<std::vector<PmRhs>> rhs(nchunk);
	for (int e = 0; e < a.nU; e++)
	{
		const int i = a.Ui[e], j = a.Uj[e];
		const bool ki = keep_pose[i] != 0, kj = keep_pose[j] != 0;
		if (!ki && !kj)
		{
			sUi.push_back(st.local[i]); sUj.push_back(st.local[j]);
			sU.insert(sU.end(), a.U + (size_t)e * 36, a.U + (size_t)e * 36 + 36);
			if (i == j) // (a diagonal block is read from its upper triangle, here as in k_pm_emit)
				for (int r = 1; r < 6; r++)
					for (int c = 0; c < r; c++) sU[sU.size() - 36 + r * 6 + c] = a.U[(size_t)e * 36 + c * 6 + r];
		}
		else if (ki != kj)
		{
			const int d = ki ? j : i, b = st.bdpos[ki ? i : j];
			rhs[b / CC_KC].push_back(PmRhs{ e, st.local[d], b % CC_KC, ki ? 1 : 0 });
		}
	}
	if (map->pose_origin) for (int p : st.dlist) sorg.push_back(map->pose_origin[p]);
	lsfm_map sub;
	memset(&sub, 0, sizeof sub);
	sub.m = nD; sub.nU = (int)sUi.size();
	sub.U = sU.data(); sub.Ui = sUi.data(); sub.Uj = sUj.data();
	sub.pose_origin = map->pose_origin ? sorg.data() : nullptr;
	// the work of k_pm_syrk: the column-tile pairs that hold at least one output pair, and where each output block finds its numbers
	std::vector<int> hbi(nout, -1), hbj(nout, -1), hwidx((size_t)nout * 4, 0);
	std::vector<unsigned long long> tiles;
	for (int e = 0; e < nout; e++)
	{
		if (!st.ofill[e]) continue;
		const int pi = hbi[e] = st.bdpos[st.klist[st.oUi[e]]], pj = hbj[e] = st.bdpos[st.klist[st.oUj[e]]];
		for (int x = (6 * pi) / 16; x <= (6 * pi + 5) / 16; x++)
			for (int y = (6 * pj) / 16; y <= (6 * pj + 5) / 16; y++)
				if (x <= y) tiles.push_back(tile_key(x, y));
	}
	std::sort(tiles.begin(), tiles.end());
	tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
	const int nwork = (int)tiles.size();
	std::vector<int2> hwork(nwork);
	for (int w = 0; w < nwork; w++) hwork[w] = make_int2((int)(tiles[w] >> 32), (int)(tiles[w] & 0xffffffffull));
	for (int e = 0; e < nout; e++)
	{
		if (hbi[e] < 0) continue;
		const int x0 = (6 * hbi[e]) / 16, y0 = (6 * hbj[e]) / 16;
		for (int x = x0; x <= (6 * hbi[e] + 5) / 16; x++)
			for (int y = y0; y <= (6 * hbj[e] + 5) / 16; y++)
				if (x <= y) hwidx[(size_t)e * 4 + (x - x0) * 2 + (y - y0)] = (int)(std::lower_bound(tiles.begin(), tiles.end(), tile_key(x, y)) - tiles.begin());
	}
	std::vector<PmRhs> hrhs;
	std::vector<int> rptr(nchunk + 1, 0);
	for (int c = 0; c < nchunk; c++)
	{
		hrhs.insert(hrhs.end(), rhs[c].begin(), rhs[c].end());
		rptr[c + 1] = (int)hrhs.size();
	}
	// ---- memory of the call ----
	const size_t NR = (size_t)nD * 6, Rtot = (size_t)nBd * 6;
	const size_t ycells = NR * Rtot;
	{
		const size_t need = (ycells + (size_t)nwork * 256 + (size_t)nout * 36 + (size_t)a.nU * 36) * sizeof(double) + (size_t)nout * 9 * sizeof(int) +
		                    hrhs.size() * sizeof(PmRhs) + (size_t)nwork * sizeof(int2);
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b)
			throw Error{ LSFM_ERR_OOM, "out of device memory: the forward-swept columns of " + std::to_string(nBd) + " boundary poses over " + std::to_string(nD) +
			                               " dropped poses need " + std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free" };
	}
	DevBuf bY, bT, bO, bU, bI, bR, bW;
	double* Y = bY.get<double>(ycells);
	double* T = bT.get<double>((size_t)nwork * 256);
	double* dO = bO.get<double>((size_t)nout * 36);
	double* dU1 = bU.get<double>((size_t)a.nU * 36);
	int* dI = bI.get<int>((size_t)nout * 9); // oUi | oUj | src | bi | bj | widx[4]
	PmRhs* dR = bR.get<PmRhs>(hrhs.size());
	int2* dW = bW.get<int2>(nwork);
	h2d(ctx, dU1, a.U, (size_t)a.nU * 36 * sizeof(double));
	h2d(ctx, dI, st.oUi.data(), (size_t)nout * sizeof(int));
	h2d(ctx, dI + nout, st.oUj.data(), (size_t)nout * sizeof(int));
	h2d(ctx, dI + 2 * (size_t)nout, st.osrc.data(), (size_t)nout * sizeof(int));
	h2d(ctx, dI + 3 * (size_t)nout, hbi.data(), (size_t)nout * sizeof(int));
	h2d(ctx, dI + 4 * (size_t)nout, hbj.data(), (size_t)nout * sizeof(int));
	h2d(ctx, dI + 5 * (size_t)nout, hwidx.data(), (size_t)nout * 4 * sizeof(int));
	h2d(ctx, dR, hrhs.data(), hrhs.size() * sizeof(PmRhs));
	h2d(ctx, dW, hwork.data(), (size_t)nwork * sizeof(int2));
	LSFM_CHECK_HIP(hipStreamSynchronize(s)); // (the staged copies have left the host vectors before cov_front reuses the ring)
	// ---- factor U1_DD ----
	CovFront fr;
	cov_front(ctx, &sub, false, fr);
	LSFM_CHECK_HIP(hipGetLastError());
	const CholDev& ch = fr.ch;
	if (info) { info[5] = ch.ntask0; info[6] = ch.ngroups; info[7] = (int)ch.glevel_ptr.size() - 1; }
	{
		const int floored = cov_front_status(ctx, fr); // throws LSFM_ERR_NOT_SPD
		if (floored > 0) return floored;                // the factor is of a perturbed U1_DD: nothing is written
	}
	// ---- right-hand sides and forward sweeps, chunk by chunk; every Y stays ----
	for (int c = 0; c < nchunk; c++)
	{
		const int kc = std::min(CC_KC, nBd - c * CC_KC), R = 6 * kc;
		double* slab = Y + (size_t)c * NR * PM_CW;
		dev_zero(ctx, slab, NR * R * sizeof(double));
		const int ne = rptr[c + 1] - rptr[c];
		if (ne) hipLaunchKernelGGL(k_pm_rhs, dim3(blocks_of((size_t)ne * 36, 256)), dim3(256), 0, s, ne, dR + rptr[c], dU1, ch.pinv, ch.dscale, R, slab);
		cc_sweep_forward(ctx, ch, R, slab);
	}
	LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	// ---- T = Y^T Y on the tile pairs, U' = U1 - T ----
	if (nwork) hipLaunchKernelGGL(k_pm_syrk, dim3(nwork), dim3(PM_WAVES * LSFM_WAVE), 0, s, dW, (int)NR, (int)Rtot, Y, T);
	hipLaunchKernelGGL(k_pm_emit, dim3(blocks_of((size_t)nout * 36, 256)), dim3(256), 0, s, nout, dI, dI + nout, dI + 2 * (size_t)nout, dI + 3 * (size_t)nout,
	                   dI + 4 * (size_t)nout, dI + 5 * (size_t)nout, dU1, T, dO);
	LSFM_CHECK_HIP(hipGetLastError());
	// ---- the map (library-allocated) ----
	const int n = a.n, nW = a.nW;
	MapOut G;
	map_new(G.g, map, nK, n, nout, nW, map->pose_origin != nullptr);
	lsfm_map& g = G.g;
	d2h(ctx, g.U, dO, (size_t)nout * 36 * sizeof(double));
	LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
	LSFM_CHECK_HIP(hipEventSynchronize(ev[3]));
	if (times)
	{
		times[0] = event_ms(ev[0], ev[1]);
		times[1] = event_ms(ev[1], fr.ev[0]);
		times[2] = event_ms(fr.ev[0], fr.ev[2]);
		times[3] = event_ms(fr.ev[2], ev[2]);
		times[4] = event_ms(ev[2], ev[3]);
	}
	memcpy(g.Ui, st.oUi.data(), (size_t)nout * sizeof(int));
	memcpy(g.Uj, st.oUj.data(), (size_t)nout * sizeof(int));
	for (int k = 0; k < nK; k++)
	{
		const int p = st.klist[k];
		memcpy(g.stno + (size_t)6 * k, a.stno + (size_t)6 * p, 6 * sizeof(int));
		memcpy(g.stVal + (size_t)6 * k, a.stVal + (size_t)6 * p, 6 * sizeof(double));
		if (g.pose_origin) g.pose_origin[k] = map->pose_origin[p];
	}
	memcpy(g.stno + (size_t)6 * nK, a.stno + (size_t)6 * m, (size_t)3 * n * sizeof(int));
	memcpy(g.stVal + (size_t)6 * nK, a.stVal + (size_t)6 * m, (size_t)3 * n * sizeof(double));
	memcpy(g.W, a.W, (size_t)nW * 18 * sizeof(double));
	memcpy(g.V, a.V, (size_t)n * 9 * sizeof(double));
	memcpy(g.feature, a.feature, (size_t)nW * sizeof(int));
	memcpy(g.FBlock, a.FBlock, (size_t)n * sizeof(int));
	for (int w = 0; w < nW; w++) g.photo[w] = st.local[a.photo[w]]; // (a kept feature is seen by kept poses alone)
	G.give(out);
	return LSFM_OK;
}

} // namespace lsfm
