// Joint compatibility of gated feature pairs: sequential selection (C ABI: lsfm_map_feature_pair_joint_gate, lsfm_selftest_pair_select).
// No reference counterpart.  The stage between the per-pair gate (lsfm_featcols.hip) and the merge (lsfm_merge.hip).
//
// The joint matrix.  A = the 3K x (6m + 3n) matrix of rows e_f - e_g, C = A Sigma A^T, d = A x^.  Column group a of the gate holds
// I^-1 (e_fa - e_ga); the feature rows of that group are Cov(x_h, x_fa - x_ga), so
//     C_ba = Sigma_{f_b,a} - Sigma_{g_b,a}
// and no column beyond the gate's 3K is solved: cc_run (lsfm_cov.hpp) with FcGroups::rhs, width 3, chunks of 64 groups.  The emit step
// takes the feature rows of the DISTINCT endpoints of all pairs with k_cc_feat<3> (a row list) and a signed-difference pass
// (k_jc_diff) rather than a kernel of k_fc_gate's shape per (pair, group): candidate lists name a feature in several pairs, the
// W-walk of a feature is then made once per chunk instead of once per pair it occurs in, and the walk itself is the kernel
// lsfm_map_covariance_feature_columns' joint already runs.  A diagonal block is overwritten with the gate's own Sigma_d (k_fc_gate: the
// sum of positive semi-definite terms), which also gives the individual d^2.  k_jc_sym applies symmetrise_joint's rule on the device.
//
// The selection.  Right-looking blocked Cholesky with rejection, in processing order, panels of JC_PP = 16 pairs = 48 columns = three
// 16-row MFMA tiles.  M[c NP + r] holds element (r, c), r >= c, of the permuted C (NP = 3K rounded up to 48, the pad zero); after the
// panels before p the trailing part is the Schur complement on the pairs accepted so far and e the conditional residual.  Per panel:
//   k_jc_panel   one work-group; the 48 x 48 diagonal block and its residuals in LDS; the pairs in turn: lane 0 asks the union-find
//                (parent[] in global memory, ordinary stores) whether the pair closes a cycle, factors the 3 x 3 block, decides; an
//                accepted pair's rank-3 update is applied inside the block by all lanes; a rejected or implied pair leaves zero columns
//   k_jc_solve   the rows below: L21 = M21 L11^-T by forward substitution, a lane per row, L11 broadcast from LDS; e2 -= L21 y1
//   k_jc_update  M22 -= L21 L21^T on v_mfma_f64_16x16x4_f64, lower-triangle tiles only, one wave per output tile, 12 steps in a fixed order
// No floating-point atomic anywhere: given the bits of C, d, the order and tau the outputs are the same bits on every call.
// Right-looking was chosen over left-looking because a decision needs the fully updated diagonal block of its pair and nothing else: the
// panel kernel then reads 48 columns, and the O(K^3) work is the one MFMA kernel with independent tiles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"

namespace lsfm {

namespace {

#define JC_PP 16          /* pairs of a panel */
#define JC_PW (3 * JC_PP) /* its columns */
#define JC_LD (JC_PW + 1) /* row stride of the panel's block in LDS */
#define JC_T 256          /* lanes of k_jc_panel and k_jc_solve */
#define JC_UW 4           /* waves of a k_jc_update work-group: an output tile each */

typedef double jc_v4d __attribute__((ext_vector_type(4)));

// C[3 b + i][3 (c0 + a) + c] = F[a][ef_b][i][c] - F[a][eg_b][i][c]: the chunk's block column against all K pairs.  F = k_cc_feat<3>'s
// out[a][E][3][3] over the E distinct endpoints, epc[2 K] the pairs' endpoints as indices into that row list.
__global__ void k_jc_diff(int K, int kcur, int c0, int E, int N3, const int* __restrict__ epc, const double* __restrict__ F, double* __restrict__ C)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)K * kcur * 9) return;
	const int c = (int)(idx % 3), a = (int)((idx / 3) % kcur), i = (int)((idx / (3 * (size_t)kcur)) % 3), b = (int)(idx / (9 * (size_t)kcur));
	const double* fa = F + (size_t)a * E * 9 + i * 3 + c;
	C[((size_t)3 * b + i) * N3 + 3 * (size_t)(c0 + a) + c] = fa[(size_t)epc[2 * b] * 9] - fa[(size_t)epc[2 * b + 1] * 9];
}
// the chunk's diagonal blocks: the gate's Sigma_d (exactly symmetric as k_fc_gate leaves it)
__global__ void k_jc_diag(int kcur, int c0, int N3, const double* __restrict__ cov, double* __restrict__ C)
{
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= kcur * 9) return;
	const int a = idx / 9, q = idx - 9 * a, i = q / 3, c = q - 3 * i;
	C[((size_t)3 * (c0 + a) + i) * N3 + 3 * (size_t)(c0 + a) + c] = cov[idx];
}
// symmetrise_joint's rule (lsfm_cov.hpp) on the device: block (a, b), a < b, from column b and mirrored; a diagonal block (X + X^T) / 2.
// The lane of (i, j), i <= j, owns both entries.
__global__ void k_jc_sym(int N3, double* __restrict__ C)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
	if (j >= N3 || i > j) return;
	const double u = C[(size_t)i * N3 + j];
	const double v = i / 3 == j / 3 ? 0.5 * (u + C[(size_t)j * N3 + i]) : u;
	C[(size_t)i * N3 + j] = v;
	C[(size_t)j * N3 + i] = v;
}

// C and d into processing order: M[c NP + r] = C[3 order[r / 3] + r % 3][3 order[c / 3] + c % 3], e[r] = d[3 order[r / 3] + r % 3]; zero
// past 3 K.  (Both triangles are filled; only r >= c is read afterwards.)
__global__ void k_jc_permute(int K, int NP, const int* __restrict__ order, const double* __restrict__ C, const double* __restrict__ d, double* __restrict__ M,
                             double* __restrict__ e)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
	if (r >= NP) return;
	const int N3 = 3 * K;
	const bool in = r < N3 && c < N3;
	const int sr = in ? 3 * order[r / 3] + r % 3 : 0, sc = in ? 3 * order[c / 3] + c % 3 : 0;
	M[(size_t)c * NP + r] = in ? C[(size_t)sr * N3 + sc] : 0.0;
	if (c == 0) e[r] = r < N3 ? d[sr] : 0.0;
}

__device__ inline int jc_find(int* parent, int x)
{
	while (parent[x] != x)
	{
		const int g = parent[parent[x]];
		parent[x] = g; // path halving
		x = g;
	}
	return x;
}

// The panel p: its pairs in turn inside the 48 x 48 diagonal block.  On exit the block's lower triangle in M holds L11 (zero columns for
// a pair that was not accepted), e[48 p ..] holds y1 = L11^-1 e1 (zero for such a pair), accP[16 p + t] says which pairs were accepted and
// pan_acc[p] how many.  statusP / deltaP in processing order.
__global__ void __launch_bounds__(JC_T) k_jc_panel(int K, int NP, int p, double tau, const int* __restrict__ endsP, const double* __restrict__ d2P,
                                                   int* __restrict__ parent, double* __restrict__ M, double* __restrict__ e, int* __restrict__ statusP,
                                                   double* __restrict__ deltaP, int* __restrict__ accP, int* __restrict__ pan_acc)
{
	__shared__ double D[JC_PW][JC_LD];
	__shared__ double ev[JC_PW];
	__shared__ double Lc[JC_PW][3];
	__shared__ double lt[6], yt[3];
	__shared__ int dec;
	const int tid = threadIdx.x, c0 = p * JC_PW;
	for (int idx = tid; idx < JC_PW * JC_PW; idx += JC_T)
	{
		const int c = idx / JC_PW, r = idx - c * JC_PW;
		if (r < c) continue;
		const double v = M[(size_t)(c0 + c) * NP + c0 + r];
		D[r][c] = v;
		D[c][r] = v;
	}
	if (tid < JC_PW) ev[tid] = e[c0 + tid];
	__syncthreads();
	int nacc = 0; // (lane 0's)
	for (int t = 0; t < JC_PP; t++)
	{
		const int pair = p * JC_PP + t, b = 3 * t;
		if (tid == 0)
		{
			int st = 0, take = 0;
			double dl = NAN;
			if (pair < K && d2P[pair] == d2P[pair])
			{
				const int f = jc_find(parent, endsP[2 * pair]), g = jc_find(parent, endsP[2 * pair + 1]);
				if (f == g) { st = 2; dl = 0.0; } // implied by the accepted pairs: nothing is factored
				else
				{
					const double p0 = D[b][b];
					if (p0 > 0.0)
					{
						const double l00 = sqrt(p0), l10 = D[b + 1][b] / l00, l20 = D[b + 2][b] / l00;
						const double p1 = D[b + 1][b + 1] - l10 * l10;
						if (p1 > 0.0)
						{
							const double l11 = sqrt(p1), l21 = (D[b + 2][b + 1] - l20 * l10) / l11;
							const double p2 = D[b + 2][b + 2] - l20 * l20 - l21 * l21;
							if (p2 > 0.0)
							{
								const double l22 = sqrt(p2);
								const double y0 = ev[b] / l00, y1 = (ev[b + 1] - l10 * y0) / l11, y2 = (ev[b + 2] - l20 * y0 - l21 * y1) / l22;
								dl = y0 * y0 + y1 * y1 + y2 * y2;
								if (dl <= tau)
								{
									st = 1; take = 1;
									parent[max(f, g)] = min(f, g);
									lt[0] = l00; lt[1] = l10; lt[2] = l11; lt[3] = l20; lt[4] = l21; lt[5] = l22;
									yt[0] = y0; yt[1] = y1; yt[2] = y2;
								}
							}
						}
					}
				}
			}
			if (pair < K) { statusP[pair] = st; deltaP[pair] = dl; }
			accP[pair] = take;
			nacc += take;
			dec = take;
		}
		__syncthreads();
		const bool below = tid > b + 2 && tid < JC_PW;
		if (dec)
		{
			if (below)
			{
				const double x0 = D[tid][b] / lt[0], x1 = (D[tid][b + 1] - x0 * lt[1]) / lt[2], x2 = (D[tid][b + 2] - x0 * lt[3] - x1 * lt[4]) / lt[5];
				Lc[tid][0] = x0; Lc[tid][1] = x1; Lc[tid][2] = x2;
			}
			__syncthreads();
			const int nb = JC_PW - (b + 3);
			for (int idx = tid; idx < nb * nb; idx += JC_T) // the rank-3 update of what is left of the block (both triangles: the same products)
			{
				const int r = b + 3 + idx / nb, c = b + 3 + idx % nb;
				D[r][c] -= fma(Lc[r][2], Lc[c][2], fma(Lc[r][1], Lc[c][1], Lc[r][0] * Lc[c][0]));
			}
			if (below)
			{
				ev[tid] -= fma(Lc[tid][2], yt[2], fma(Lc[tid][1], yt[1], Lc[tid][0] * yt[0]));
				D[tid][b] = Lc[tid][0]; D[tid][b + 1] = Lc[tid][1]; D[tid][b + 2] = Lc[tid][2]; // the columns of L11 (the update is to their right)
			}
			if (tid == 0)
			{
				D[b][b] = lt[0]; D[b + 1][b] = lt[1]; D[b + 1][b + 1] = lt[2]; D[b + 2][b] = lt[3]; D[b + 2][b + 1] = lt[4]; D[b + 2][b + 2] = lt[5];
				ev[b] = yt[0]; ev[b + 1] = yt[1]; ev[b + 2] = yt[2];
			}
		}
		else
		{
			if (tid >= b && tid < JC_PW) { D[tid][b] = 0.0; D[tid][b + 1] = 0.0; D[tid][b + 2] = 0.0; }
			if (tid < 3) ev[b + tid] = 0.0;
		}
		__syncthreads();
	}
	for (int idx = tid; idx < JC_PW * JC_PW; idx += JC_T)
	{
		const int c = idx / JC_PW, r = idx - c * JC_PW;
		if (r >= c) M[(size_t)(c0 + c) * NP + c0 + r] = D[r][c];
	}
	if (tid < JC_PW) e[c0 + tid] = ev[tid];
	if (tid == 0) pan_acc[p] = nacc;
}

// The rows below panel p, a lane per row r: x = M[r][panel] L11^-T by forward substitution over the 48 columns (a column of a pair that was
// not accepted gives 0), written back in place; e[r] -= x . y1.  L11 and y1 are broadcast from LDS.  Nothing to do where the panel accepted
// no pair: its columns are never read again.
__global__ void __launch_bounds__(JC_T) k_jc_solve(int NP, int p, const int* __restrict__ accP, const int* __restrict__ pan_acc, double* __restrict__ M,
                                                   double* __restrict__ e)
{
	__shared__ double L[JC_PW][JC_LD];
	__shared__ double y[JC_PW];
	__shared__ int ok[JC_PW];
	if (!pan_acc[p]) return;
	const int tid = threadIdx.x, c0 = p * JC_PW;
	for (int idx = tid; idx < JC_PW * JC_PW; idx += JC_T)
	{
		const int c = idx / JC_PW, r = idx - c * JC_PW;
		L[r][c] = r >= c ? M[(size_t)(c0 + c) * NP + c0 + r] : 0.0;
	}
	if (tid < JC_PW)
	{
		y[tid] = e[c0 + tid];
		ok[tid] = accP[p * JC_PP + tid / 3];
	}
	__syncthreads();
	const int r = c0 + JC_PW + blockIdx.x * JC_T + tid;
	if (r >= NP) return;
	double x[JC_PW];
	double* col = M + (size_t)c0 * NP + r;
#pragma unroll
	for (int c = 0; c < JC_PW; c++)
	{
		double v = col[(size_t)c * NP];
#pragma unroll
		for (int k = 0; k < c; k++) v = fma(-x[k], L[c][k], v);
		x[c] = ok[c] ? v / L[c][c] : 0.0;
	}
	double s = e[r];
#pragma unroll
	for (int c = 0; c < JC_PW; c++)
	{
		col[(size_t)c * NP] = x[c];
		s = fma(-x[c], y[c], s);
	}
	e[r] = s;
}

// M22 -= L21 L21^T behind panel p, the tiles (rt >= ct) of the lower triangle alone, one wave per output tile.  The tile is taken
// transposed -- A from the rows of ct, B from the rows of rt -- so that with the f64 MFMA's C/D layout (col = lane & 15, row = (lane >> 4)
// + 4 reg) register reg of lane l is element (row 16 rt + (l & 15), column 16 ct + (l >> 4) + 4 reg): 16 consecutive doubles of M per
// quarter wave, and both operands load 16 consecutive doubles of a column of L as well.  12 steps of 4 columns in ascending order.
// A diagonal tile (rt == ct) is written whole: its strict upper part (r < c) lands in slots of M that k_jc_permute filled and nothing reads
// afterwards -- M is read as lower-triangle storage only, the stores above the diagonal are harmless and cheaper than a mask.
__global__ void __launch_bounds__(JC_UW * LSFM_WAVE) k_jc_update(int NP, int p, const int* __restrict__ pan_acc, double* __restrict__ M)
{
	if (!pan_acc[p]) return;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
	const int tb = (p + 1) * (JC_PW / 16);
	const int rt = tb + blockIdx.y, ct = tb + blockIdx.x * JC_UW + wave;
	if (ct > rt) return;
	const double* pa = M + (size_t)(p * JC_PW + kq) * NP + ct * 16 + cl;
	const double* pb = M + (size_t)(p * JC_PW + kq) * NP + rt * 16 + cl;
	jc_v4d acc = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
	for (int ks = 0; ks < JC_PW / 4; ks++)
	{
		const double a = pa[(size_t)ks * 4 * NP], b = pb[(size_t)ks * 4 * NP];
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
	}
#pragma unroll
	for (int reg = 0; reg < 4; reg++)
	{
		double* o = M + (size_t)(ct * 16 + kq + 4 * reg) * NP + rt * 16 + cl;
		*o -= acc[reg];
	}
}

inline unsigned jc_blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// the individual d^2 of a 3 x 3 block (lower triangle) as k_fc_gate takes it
double jc_host_d2(const double* C, size_t ld, const double* x)
{
	const double p0 = C[0];
	if (!(p0 > 0.0)) return NAN;
	const double l00 = std::sqrt(p0), l10 = C[ld] / l00, l20 = C[2 * ld] / l00;
	const double p1 = C[ld + 1] - l10 * l10;
	if (!(p1 > 0.0)) return NAN;
	const double l11 = std::sqrt(p1), l21 = (C[2 * ld + 1] - l20 * l10) / l11;
	const double p2 = C[2 * ld + 2] - l20 * l20 - l21 * l21;
	if (!(p2 > 0.0)) return NAN;
	const double l22 = std::sqrt(p2);
	const double y0 = x[0] / l00, y1 = (x[1] - l10 * y0) / l11, y2 = (x[2] - l20 * y0 - l21 * y1) / l22;
	return y0 * y0 + y1 * y1 + y2 * y2;
}

void jc_check_args(int K, const int* order, double tau)
{
	if (K < 1 || K > LSFM_JOINT_GATE_MAX) LSFM_FAIL(LSFM_ERR_ARG, "K = " + std::to_string(K) + " pairs: 1 <= K <= " + std::to_string(LSFM_JOINT_GATE_MAX));
	if (!(tau > 0.0)) LSFM_FAIL(LSFM_ERR_ARG, "tau must be > 0 (+inf is allowed)");
	if (!order) return;
	std::vector<char> seen(K, 0);
	for (int a = 0; a < K; a++)
	{
		if (order[a] < 0 || order[a] >= K || seen[order[a]]) LSFM_FAIL(LSFM_ERR_ARG, "order is not a permutation of 0.." + std::to_string(K - 1) + " (entry " + std::to_string(a) + ")");
		seen[order[a]] = 1;
	}
}

// The selection on the device.  dC [(3K)^2] symmetric and dd [3K] on the device in input order; h_d2[K] the individual d^2 (host; NaN = the
// pair is rejected unseen, and the default order); ends[2K] any labels of the pairs' endpoints; order_in may be null.  Outputs in input order.
// kev (may be null): two events, recorded in front of k_jc_permute and behind the last panel -- the kernels of the selection and nothing else.
void jc_select(lsfm_context* ctx, int K, const double* dC, const double* dd, const double* h_d2, const int* ends, const int* order_in, double tau, int* status,
               double* delta, double* D2, int* accepted, int* implied, hipEvent_t* kev = nullptr)
{
	hipStream_t s = ctx->stream;
	const int npan = (K + JC_PP - 1) / JC_PP, NP = npan * JC_PW, KP = npan * JC_PP;
	std::vector<int> order(K);
	if (order_in) std::copy(order_in, order_in + K, order.begin());
	else
	{
		// ascending d2, ties by input index, NaN last: a function of the bits of d2 alone
		std::iota(order.begin(), order.end(), 0);
		std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
			const bool na = std::isnan(h_d2[a]), nb = std::isnan(h_d2[b]);
			return na != nb ? nb : (!na && h_d2[a] < h_d2[b]);
		});
	}
	// the endpoints as 0..E-1, in processing order
	std::vector<int> lab(ends, ends + 2 * (size_t)K);
	std::sort(lab.begin(), lab.end());
	lab.erase(std::unique(lab.begin(), lab.end()), lab.end());
	const int E = (int)lab.size();
	std::vector<int> endsP(2 * (size_t)KP, 0), parent(E);
	std::vector<double> d2P(KP, NAN);
	std::iota(parent.begin(), parent.end(), 0);
	for (int a = 0; a < K; a++)
	{
		const int b = order[a];
		for (int side = 0; side < 2; side++) endsP[2 * (size_t)a + side] = (int)(std::lower_bound(lab.begin(), lab.end(), ends[2 * (size_t)b + side]) - lab.begin());
		d2P[a] = h_d2[b];
	}
	DevBuf bM, bE, bO, bN, bD, bP, bS, bL, bA, bT;
	double* M = bM.get<double>((size_t)NP * NP);
	double* e = bE.get<double>(NP);
	int* dorder = bO.get<int>(K);
	int* dends = bN.get<int>(2 * (size_t)KP);
	double* dd2 = bD.get<double>(KP);
	int* dparent = bP.get<int>(E);
	int* dstatus = bS.get<int>(KP);
	double* ddelta = bL.get<double>(KP);
	int* dacc = bA.get<int>(KP);
	int* dpan = bT.get<int>(npan);
	h2d(ctx, dorder, order.data(), (size_t)K * sizeof(int));
	h2d(ctx, dends, endsP.data(), 2 * (size_t)KP * sizeof(int));
	h2d(ctx, dd2, d2P.data(), (size_t)KP * sizeof(double));
	h2d(ctx, dparent, parent.data(), (size_t)E * sizeof(int));
	if (kev) LSFM_CHECK_HIP(hipEventRecord(kev[0], s));
	hipLaunchKernelGGL(k_jc_permute, dim3(jc_blocks(NP, 256), NP), dim3(256), 0, s, K, NP, dorder, dC, dd, M, e);
	for (int p = 0; p < npan; p++)
	{
		hipLaunchKernelGGL(k_jc_panel, dim3(1), dim3(JC_T), 0, s, K, NP, p, tau, dends, dd2, dparent, M, e, dstatus, ddelta, dacc, dpan);
		const int below = NP - (p + 1) * JC_PW;
		if (!below) break;
		hipLaunchKernelGGL(k_jc_solve, dim3(jc_blocks(below, JC_T)), dim3(JC_T), 0, s, NP, p, dacc, dpan, M, e);
		const int T = below / 16;
		hipLaunchKernelGGL(k_jc_update, dim3(jc_blocks(T, JC_UW), T), dim3(JC_UW * LSFM_WAVE), 0, s, NP, p, dpan, M);
	}
	if (kev) LSFM_CHECK_HIP(hipEventRecord(kev[1], s));
	LSFM_CHECK_HIP(hipGetLastError());
	std::vector<int> hs(KP);
	std::vector<double> hd(KP);
	d2h(ctx, hs.data(), dstatus, (size_t)K * sizeof(int));
	d2h(ctx, hd.data(), ddelta, (size_t)K * sizeof(double));
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	double sum = 0.0;
	int na = 0, ni = 0;
	for (int a = 0; a < K; a++) // processing order: the sum is that of the factorisation
	{
		status[order[a]] = hs[a];
		delta[order[a]] = hd[a];
		if (hs[a] == 1) { sum += hd[a]; na++; }
		else if (hs[a] == 2) ni++;
	}
	if (D2) *D2 = sum;
	if (accepted) *accepted = na;
	if (implied) *implied = ni;
}

} // namespace

int map_feature_pair_joint_gate(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, const int* order, double tau, int* status,
                                double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps_out, double* last_corr, double* times)
{
	jc_check_args(K, order, tau);
	const int m = map->m, n = map->n;
	std::vector<int> grp(pairs, pairs + 2 * (size_t)K);
	std::vector<double> dx(3 * (size_t)K);
	for (int a = 0; a < K; a++)
	{
		const int f = grp[2 * a], g = grp[2 * a + 1];
		if (f < 0 || f >= n || g < 0 || g >= n) LSFM_FAIL(LSFM_ERR_ARG, "pair " + std::to_string(a) + " (" + std::to_string(f) + ", " + std::to_string(g) + ") names a feature that is not one of the map's " + std::to_string(n));
		if (f == g) LSFM_FAIL(LSFM_ERR_ARG, "pair " + std::to_string(a) + " names feature " + std::to_string(f) + " twice");
		for (int i = 0; i < 3; i++) dx[3 * (size_t)a + i] = map->stVal[(size_t)6 * m + 3 * (size_t)f + i] - map->stVal[(size_t)6 * m + 3 * (size_t)g + i];
	}
	// the distinct endpoints: the row list of the feature kernel, and the pairs' endpoints as indices into it
	std::vector<int> rows(grp);
	std::sort(rows.begin(), rows.end());
	rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
	const int E = (int)rows.size(), N3 = 3 * K;
	std::vector<int> epc(2 * (size_t)K);
	for (size_t i = 0; i < epc.size(); i++) epc[i] = (int)(std::lower_bound(rows.begin(), rows.end(), grp[i]) - rows.begin());
	const int kc = std::min(K, 2 * CC_KC);
	const size_t nF = (size_t)kc * E * 9, nC = (size_t)N3 * N3;
	FcGroups dg;
	DevBuf bX, bD, bV, bR, bQ, bF, bC;
	double *ddx = nullptr, *dd2 = nullptr, *dcov = nullptr, *F = nullptr, *dC = nullptr;
	int *drows = nullptr, *depc = nullptr;
	int own_steps = 0;
	int& steps = steps_out ? *steps_out : own_steps;
	double t4[4] = { 0, 0, 0, 0 };
	// (the selection's own copy of C in processing order is counted with the call's outputs)
	const int rc = cc_run(ctx, map, mono, CcCall{ K, 3, 2 * CC_KC, nF + 2 * nC + 24 * (size_t)K, "pairs" }, &steps, last_corr, t4,
		[&](const CovFront&) {
			dg.upload(ctx, grp);
			ddx = bX.get<double>(3 * (size_t)K);
			h2d(ctx, ddx, dx.data(), 3 * (size_t)K * sizeof(double));
			dd2 = bD.get<double>(K);
			dcov = bV.get<double>(9 * (size_t)kc);
			drows = bR.get<int>(E);
			h2d(ctx, drows, rows.data(), (size_t)E * sizeof(int));
			depc = bQ.get<int>(2 * (size_t)K);
			h2d(ctx, depc, epc.data(), 2 * (size_t)K * sizeof(int));
			F = bF.get<double>(nF);
			dC = bC.get<double>(nC);
		},
		dg.rhs(ctx), nullptr,
		[&](int c0, int kcur, int R, const CovFront& fr, CcWork& wk) {
			fc_gate(ctx, fr, R, kcur, dg.of(c0), wk.Xo, ddx + 3 * (size_t)c0, dd2 + c0, dcov);
			cc_feat(ctx, 3, fr, R, drows, E, dg.of(c0), wk.Xo, F);
			hipLaunchKernelGGL(k_jc_diff, dim3(jc_blocks((size_t)K * kcur * 9, 256)), dim3(256), 0, ctx->stream, K, kcur, c0, E, N3, depc, F, dC);
			hipLaunchKernelGGL(k_jc_diag, dim3(jc_blocks((size_t)kcur * 9, 256)), dim3(256), 0, ctx->stream, kcur, c0, N3, dcov, dC);
		},
		[&](int, int, int, CcWork&) {});
	if (rc > 0 && steps == 0) return rc; // floored pivots: nothing was run, nothing is written
	hipStream_t s = ctx->stream;
	hipEvent_t ev[3] = { ctx->pool_event(), ctx->pool_event(), ctx->pool_event() }, kev[2] = { ctx->pool_event(), ctx->pool_event() };
	LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	hipLaunchKernelGGL(k_jc_sym, dim3(jc_blocks(N3, 256), N3), dim3(256), 0, s, N3, dC);
	LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	std::vector<double> hd2(K);
	d2h(ctx, hd2.data(), dd2, (size_t)K * sizeof(double));
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	jc_select(ctx, K, dC, ddx, hd2.data(), grp.data(), order, tau, status, delta, D2, accepted, implied, kev);
	if (d2) memcpy(d2, hd2.data(), (size_t)K * sizeof(double));
	if (joint_C) d2h(ctx, joint_C, dC, nC * sizeof(double));
	LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	if (times)
	{
		times[0] = t4[0]; times[1] = t4[1]; times[2] = t4[2];
		times[3] = t4[3] + event_ms(ev[0], ev[1]);
		times[4] = event_ms(kev[0], kev[1]);                             // k_jc_permute .. the last panel
		times[5] = event_ms(ev[1], kev[0]) + event_ms(kev[1], ev[2]);    // d2 down, order + endpoints + allocations, status / delta / C down
	}
	return rc;
}

int pair_select_selftest(lsfm_context* ctx, int K, const double* C, const double* d, const int* ends, const int* order, double tau, int* status, double* delta,
                         double* D2, int* accepted, int* implied)
{
	jc_check_args(K, order, tau);
	for (int a = 0; a < K; a++)
		if (ends[2 * a] == ends[2 * a + 1]) LSFM_FAIL(LSFM_ERR_ARG, "pair " + std::to_string(a) + " names endpoint " + std::to_string(ends[2 * a]) + " twice");
	const size_t N3 = 3 * (size_t)K;
	std::vector<double> hd2(K);
	for (int a = 0; a < K; a++) hd2[a] = jc_host_d2(C + (3 * (size_t)a) * N3 + 3 * (size_t)a, N3, d + 3 * (size_t)a);
	DevBuf bC, bD;
	double* dC = bC.get<double>(N3 * N3);
	double* dd = bD.get<double>(N3);
	h2d(ctx, dC, C, N3 * N3 * sizeof(double));
	h2d(ctx, dd, d, N3 * sizeof(double));
	jc_select(ctx, K, dC, dd, hd2.data(), ends, order, tau, status, delta, D2, accepted, implied);
	return LSFM_OK;
}

} // namespace lsfm
