// Batched Schur complement + preconditioned CG + back-substitution for all joins of one tree level.
// Replaces lmj_solveLinearSFM{Stereo,Mono} (Imp.cpp:2119-2378 / 6756-7041): the reference builds S = U - W V^-1 W^T
// through a dense m x m byte mask and hands it to CHOLMOD; here
//   K7  k_vinv            V^-1 per feature                                   (pba_inverseV, Imp.cpp:3022-3042)
//   K8  (lsfm_pattern.hip) block pattern of S by hashing the pose pairs that share a feature + U's pattern, sorted into block CSR
//   K9  k_schur_*         S(p,q) -= W_pf V_f^-1 W_qf^T, E_p -= W_pf V_f^-1 eb_f (Imp.cpp:2244-2332): k_schur_panel
//                         (lsfm_schur_panel.hip, fp64 MFMA on 128-feature tiles); k_schur_w here takes the tiles it flags
//   K10 k_spmv / k_pcg_*  Cholesky-preconditioned CG (lsfm_pcg.hip; the factor: lsfm_chol.hip) on the symmetric 6x6-block system, all independent
//                         systems of the level together with per-system scalars (replaces Imp.cpp:2334-2361)
//   K11 k_backsub         features: x_f = V_f^-1 (eb_f - sum W_pf^T x_p)     (pba_solveFeatures, Imp.cpp:2980-3020)
// S is kept as its upper block triangle (diagonal blocks full); the SpMV reads every stored block once and adds its
// mirrored part through an LDS window of y (k_spmv).
#include <algorithm>
#include <cmath>

#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

// also what the panel kernel of K9 needs per feature: V^-1 = L L^T (l00 l10 l11 l20 l21 l22) and y = L^T eb, so that its
// passes find them ready instead of running a Cholesky with square roots and divisions on a dependent load each;
// l00 = NaN marks a V^-1 without a Cholesky factor (the tile then goes to k_schur_w)
// ymax (optional): per work-group the largest |L^T eb|^2 of its features -- what bounds K9's right-hand-side sums (k_schur_scale)
// rhs (fused right-hand side): eb is the V part only; also leaves uu = [L^-1 x_f of the End source | of the Cur source]
__global__ void __launch_bounds__(256) k_vinv(int NF, const double* __restrict__ V, const double* __restrict__ eb, double* __restrict__ IV, double* __restrict__ LY,
                                               double* __restrict__ ymax, RhsFused rhs, double* __restrict__ uu)
{
	__shared__ double wmax[4];
	// V, eb in and V^-1, (L, y) out as the work-group's contiguous ranges (tile_records_*): one tile for the 9-double records in turn
	__shared__ double sRec[256 * 9], sEb[256 * 3];
	const int f0 = blockIdx.x * 256, nrec = min(256, NF - f0);
	int f = f0 + threadIdx.x;
	tile_records_load<9>(sRec, V + (size_t)f0 * 9, nrec);
	tile_records_load<3>(sEb, eb + (size_t)f0 * 3, nrec);
	__syncthreads();
	double y2 = 0.0;
	double* rec = sRec + threadIdx.x * 9;
	double l[9];
	if (f < NF)
	{
	double a[9], o[9];
	ld<9>(a, rec);
	inv3_sym(a, o);
	st<9>(rec, o);
	const double* e = sEb + threadIdx.x * 3;
	const double d0 = o[0];
	l[0] = sqrt(d0);
	l[1] = o[3] / l[0];
	l[3] = o[6] / l[0];
	const double d1 = o[4] - l[1] * l[1];
	l[2] = sqrt(d1);
	l[4] = (o[7] - l[3] * l[1]) / l[2];
	const double d2 = o[8] - l[3] * l[3] - l[4] * l[4];
	l[5] = sqrt(d2);
	l[6] = l[0] * e[0] + l[1] * e[1] + l[3] * e[2];
	l[7] = l[2] * e[1] + l[4] * e[2];
	l[8] = l[5] * e[2];
	if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) l[0] = __builtin_nan("");
	y2 = l[6] * l[6] + l[7] * l[7] + l[8] * l[8];
	if (uu)
	{
#pragma unroll
		for (int sd = 0; sd < 2; sd++)
		{
			const int fs = sd ? rhs.srcC[f] : rhs.srcE[f];
			double u0 = 0.0, u1 = 0.0, u2 = 0.0;
			if (fs >= 0)
			{
				const double* x = rhs.feat_src + (size_t)fs * 3;
				u0 = x[0] / l[0];
				u1 = (x[1] - l[1] * u0) / l[2];
				u2 = (x[2] - l[3] * u0 - l[4] * u1) / l[5];
			}
			uu[(size_t)f * 6 + 3 * sd] = u0; uu[(size_t)f * 6 + 3 * sd + 1] = u1; uu[(size_t)f * 6 + 3 * sd + 2] = u2;
			y2 = fmax(y2, u0 * u0 + u1 * u1 + u2 * u2);
		}
	}
	if (!(y2 == y2)) y2 = 0.0; // (a feature without a factor goes to k_schur_w, which checks its own sums)
	}
	__syncthreads();
	tile_records_store<9>(sRec, IV + (size_t)f0 * 9, nrec);
	__syncthreads();
	if (f < NF) st<9>(rec, l);
	__syncthreads();
	tile_records_store<9>(sRec, LY + (size_t)f0 * 9, nrec);
	if (!ymax) return;
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) y2 = fmax(y2, __shfl_xor(y2, off, LSFM_WAVE));
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) wmax[threadIdx.x >> 6] = y2;
	__syncthreads();
	if (threadIdx.x == 0) ymax[blockIdx.x] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
}

// The scales of K9's fixed-point sums.  Per pose scalar i: sexp[i] with 2^sexp[i] > 2 sqrt(U_ii), U_ii the diagonal entry of the
// camera block of the joint information matrix (k_schur_u has put U into S: the diagonal block is the first of its row).  S = U - W
// V^-1 W^T is a Schur complement of a positive semi-definite matrix, so every partial sum over features of (W V^-1 W^T)_ij stays below
// sqrt(U_ii U_jj) (Cauchy-Schwarz on the semi-definite partial sums) -- known BEFORE K9 runs.  sexp[6 M] = ey with
// 2^ey > 2 sqrt(NF max_f |L_f^T eb_f|^2) >= 2 |L^T eb|: |(W V^-1 eb)_i| = |(W L)(L^T eb)|_i <= sqrt(U_ii) |L^T eb|.
__device__ __forceinline__ int half_exponent(double d) // smallest-ish e with 2^e > 2 sqrt(d); 0 for d <= 0 (an empty row: nothing is ever added)
{
	if (!(d > 0.0) || !(d < 1e300)) return 0;
	int k;
	(void)frexp(d, &k); // d = f 2^k, 1/2 <= f < 1: sqrt(d) < 2^((k + 1) >> 1)
	return ((k + 1) >> 1) + 1;
}
__global__ void __launch_bounds__(256) k_schur_scale(int M, const int* __restrict__ rowptr, const double* __restrict__ S, int NF, int nymax,
                                                      const double* __restrict__ ymax, const unsigned char* __restrict__ fixed, int* __restrict__ sexp,
                                                      const double* __restrict__ ea, double* __restrict__ E)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < 6 * M)
	{
		E[i] = ea[i]; // (the right-hand side starts as its pose part: a copy of its own until round 5)
		const int p = i / 6, r = i - 6 * p;
		// (a scalar removed from the system -- the Mono gauge -- has no bound and needs none: a scale beyond every addend, whatever lands
		// in its row and column rounds to nothing)
		sexp[i] = (fixed && fixed[i]) ? 400 : half_exponent(S[(size_t)rowptr[p] * 36 + 7 * r]);
	}
	if (blockIdx.x == 0)
	{
		__shared__ double wmax[4];
		double m = 0.0;
		for (int b = threadIdx.x; b < nymax; b += 256) m = fmax(m, ymax[b]);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, LSFM_WAVE));
		if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) wmax[threadIdx.x >> 6] = m;
		__syncthreads();
		// (+ 20: with the fused right-hand side y gains P^T x_p, of the size of L^T eb but not bounded by it -- two limbs leave 100 bits)
		if (threadIdx.x == 0) sexp[6 * (size_t)M] = half_exponent((double)NF * fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]))) + 20;
	}
}
// S -= (the integer sums of W V^-1 W^T); E += (the two limbs of -W V^-1 eb); a poisoned level leaves NaN everywhere (its
// factorisation then reports the system, as a NaN in a floating-point sum did)
__global__ void k_schur_finish(int nnzb, int M, const unsigned long long* __restrict__ keys, const long long* __restrict__ acc, const int* __restrict__ sexp,
                               double* __restrict__ S, double* __restrict__ E)
{
	// acc: [poison word | nnzb * 36 sums of W V^-1 W^T | 6 M high limbs | 6 M low limbs]
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t ns = (size_t)nnzb * 36, ne = (size_t)M * 6;
	const bool poison = acc[0] != 0;
	acc += 1;
	if (i < ns)
	{
		const unsigned long long key = keys[i / 36];
		const int p = (int)(key >> 32), q = (int)(key & 0xffffffffull), rc = (int)(i % 36);
		const double v = ldexp((double)acc[i], sexp[6 * (size_t)p + rc / 6] + sexp[6 * (size_t)q + rc % 6] - 60);
		S[i] = poison ? __builtin_nan("") : S[i] - v;
	}
	else if (i < ns + ne)
	{
		const size_t k = i - ns;
		const int e = sexp[k] + sexp[ne] - 62;
		const double v = ldexp((double)acc[ns + k], e) + ldexp((double)acc[ns + ne + k], e - 40);
		E[k] = poison ? __builtin_nan("") : E[k] + v;
	}
}

// sum over the features of (run length)^2: the pose pairs of K9 (for its algorithmic flop count)
__global__ void __launch_bounds__(256) k_sum_run_squares(int NF, const int* __restrict__ fptr, unsigned long long* out)
{
	// a few hundred work-groups striding over the features, ONE atomic each (one per wave on a single address took 120 us)
	__shared__ unsigned long long part[4];
	unsigned long long v = 0;
	for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < NF; f += gridDim.x * blockDim.x)
	{
		const unsigned long long k = (unsigned long long)(fptr[f + 1] - fptr[f]);
		v += k * k;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, LSFM_WAVE);
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) part[threadIdx.x >> 6] = v;
	__syncthreads();
	if (threadIdx.x == 0) { v = part[0] + part[1] + part[2] + part[3]; if (v) atomicAdd(out, v); }
}

// ---- numeric Schur complement ------------------------------------------------------------------------------
// (one lane per block looks its place in S up; the 36 numbers of the work-group's blocks then leave by consecutive lanes on consecutive
// numbers -- one lane per block adding its 36 at a stride of 288 bytes was 63 us for the 37 MB of U at the top of an NC3500-like tree)
#define SCHUR_U_BLOCKS 256
__global__ void __launch_bounds__(SCHUR_U_BLOCKS) k_schur_u(int NU, const double* __restrict__ U, const int* __restrict__ Ui, const int* __restrict__ Uj,
                                                          const unsigned long long* __restrict__ tab, const int* __restrict__ val, unsigned long long mask,
                                                          double* __restrict__ S)
{
	__shared__ int s_slot[SCHUR_U_BLOCKS]; // slot of S, | 1 << 30: the block goes in transposed
	const int i0 = blockIdx.x * SCHUR_U_BLOCKS, nb = min(SCHUR_U_BLOCKS, NU - i0);
	if ((int)threadIdx.x < nb)
	{
		const int a = Ui[i0 + threadIdx.x], b = Uj[i0 + threadIdx.x];
		const int slot = hash_find(tab, val, mask, pair_key(a, b));
		s_slot[threadIdx.x] = slot < 0 ? -1 : (slot | (a <= b ? 0 : (1 << 30)));
	}
	__syncthreads();
	const double* u = U + (size_t)i0 * 36;
	for (int p = threadIdx.x; p < nb * 36; p += SCHUR_U_BLOCKS)
	{
		const int blk = p / 36, q = p - 36 * blk, sl = s_slot[blk];
		if (sl < 0) continue;
		const int slot = sl & ((1 << 30) - 1);
		const int qq = (sl >> 30) ? (q % 6) * 6 + q / 6 : q; // (u[r][c] -> s[c][r])
		atomic_add_f64(S + (size_t)slot * 36 + qq, u[p]);
	}
}

// K9, one lane per feature.  A tile of SCHUR_TILE consecutive features (one work-group) touches few distinct blocks
// of S (its ~10 hub poses squared plus the handful of poses that observe the tile), while every feature contributes
// k_f(k_f+1)/2 of them: all contributions are first summed in an LDS table keyed by the block's slot (ds_add_f64) and
// each touched block leaves the work-group once, as 36 contiguous atomics.  (Scattering 8-byte atomics straight to HBM
// ran at ~0.08 TB/s, MI355X_MICROARCH "Global float atomics": 64 lanes in 64 different rows.)
#define SCHUR_TILE 128
#define SCHUR_CAP 256 /* LDS block accumulators per work-group: 256 * 288 B = 72 KiB -> 2 work-groups per CU */
#define SCHUR_ECAP 64 /* LDS accumulators for E (per pose) */

__global__ void __launch_bounds__(SCHUR_TILE)
k_schur_w(int NF, const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W, const double* __restrict__ IV,
          const double* __restrict__ eb, const unsigned long long* __restrict__ tab, const int* __restrict__ val, unsigned long long mask,
          K9Out o, const unsigned char* __restrict__ only, const double* __restrict__ LY)
{
	if (only && !only[blockIdx.x / (LSFM_PM_TILE / SCHUR_TILE)]) return; // fallback pass: only the tiles the panel kernel could not take
	// (the same fixed-point sums as the panel kernel's, k_schur_scale: per feature here, so already the LDS tables are integers)
	__shared__ int skey[SCHUR_CAP];
	__shared__ int ekey[SCHUR_ECAP];
	__shared__ long long sval[SCHUR_CAP * 36];
	__shared__ long long evalv[SCHUR_ECAP * 12]; // high limbs, then low limbs
	const int tid = threadIdx.x;
	for (int i = tid; i < SCHUR_CAP; i += SCHUR_TILE) skey[i] = -1;
	for (int i = tid; i < SCHUR_ECAP; i += SCHUR_TILE) ekey[i] = -1;
	for (int i = tid; i < SCHUR_CAP * 36; i += SCHUR_TILE) sval[i] = 0;
	for (int i = tid; i < SCHUR_ECAP * 12; i += SCHUR_TILE) evalv[i] = 0;
	__syncthreads();
	const int f = blockIdx.x * SCHUR_TILE + tid;
	bool bad = false;
	const int ey = *o.ey;
	if (f < NF)
	{
		const int j0 = fptr[f], len = fptr[f + 1] - j0;
		double iv[9];
		ld<9>(iv, IV + (size_t)f * 9);
		double eb0 = eb[(size_t)f * 3], eb1 = eb[(size_t)f * 3 + 1], eb2 = eb[(size_t)f * 3 + 2];
		double xfs[2][3] = { { 0.0, 0.0, 0.0 }, { 0.0, 0.0, 0.0 } };
		if (o.xpose)
		{
			// fused right-hand side (K9Out): eb += W^T x_p over the run; the feature's estimate in either source map = L u
			for (int a = 0; a < len; a++)
			{
				const double* wa = W + (size_t)(j0 + a) * 18;
				const double* xp = o.xpose + (size_t)photo[j0 + a] * 6;
#pragma unroll
				for (int r = 0; r < 6; r++) { eb0 = fma(wa[3 * r], xp[r], eb0); eb1 = fma(wa[3 * r + 1], xp[r], eb1); eb2 = fma(wa[3 * r + 2], xp[r], eb2); }
			}
			const double* l = LY + (size_t)f * 9;
			if (!(l[0] == l[0])) bad = true; // (V^-1 without a factor: no y to leave -- the level is reported, as a NaN in S would be)
#pragma unroll
			for (int sd = 0; sd < 2; sd++)
			{
				const double* u = o.uu + (size_t)f * 6 + 3 * sd;
				xfs[sd][0] = l[0] * u[0]; xfs[sd][1] = l[1] * u[0] + l[2] * u[1]; xfs[sd][2] = l[3] * u[0] + l[4] * u[1] + l[5] * u[2];
			}
		}
		for (int a = 0; a < len; a++)
		{
			double WV[18], Wa[18];
			const int pa = photo[j0 + a];
			ld<18>(Wa, W + (size_t)(j0 + a) * 18);
			mm<6, 3, 3, false>(Wa, iv, WV); // W V^-1 (V^-1 symmetric), Imp.cpp:2260-2273
			int ea6[6];
#pragma unroll
			for (int r = 0; r < 6; r++) ea6[r] = o.sexp[(size_t)pa * 6 + r];
			{
				// E_p -= W V^-1 eb, Imp.cpp:2321-2328
				const int es = lds_slot(ekey, SCHUR_ECAP, pa);
#pragma unroll
				for (int r = 0; r < 6; r++)
				{
					double e = -(WV[3 * r] * eb0 + WV[3 * r + 1] * eb1 + WV[3 * r + 2] * eb2);
					if (o.xpose) { const double* xf = xfs[o.pside[pa] & 1]; e += Wa[3 * r] * xf[0] + Wa[3 * r + 1] * xf[1] + Wa[3 * r + 2] * xf[2]; }
					long long hi, lo;
					to_fixed2(e, 62 - ea6[r] - ey, hi, lo, bad);
					if (es >= 0) { lds_add_i64(&evalv[es * 6 + r], hi); lds_add_i64(&evalv[SCHUR_ECAP * 6 + es * 6 + r], lo); }
					else { atomic_add_i64(o.Ehi + (size_t)pa * 6 + r, hi); atomic_add_i64(o.Elo + (size_t)pa * 6 + r, lo); }
				}
			}
			for (int b = a; b < len; b++)
			{
				double Wb[18], T[36];
				const int pb = photo[j0 + b];
				ld<18>(Wb, W + (size_t)(j0 + b) * 18);
				mmt<6, 3, 6, false>(WV, Wb, T); // W_a V^-1 W_b^T = contribution to S(pa,pb), Imp.cpp:2283-2318
				const int slot = hash_find(tab, val, mask, pair_key(pa, pb));
				const int ls = lds_slot(skey, SCHUR_CAP, slot);
				long long* dl = ls >= 0 ? &sval[ls * 36] : nullptr;
				long long* dg = o.S + (size_t)slot * 36;
				int eb6[6];
#pragma unroll
				for (int c = 0; c < 6; c++) eb6[c] = o.sexp[(size_t)pb * 6 + c];
				// stored orientation: rows = the smaller pose index; a block of one pose with itself is stored full
				const bool same = (pa == pb), tr = pa > pb, twice = same && a != b;
#pragma unroll
				for (int r = 0; r < 6; r++)
#pragma unroll
					for (int c = 0; c < 6; c++)
					{
						// (+: the accumulators hold W V^-1 W^T, k_schur_finish subtracts)
						double x = T[r * 6 + c];
						if (twice) x += T[c * 6 + r];
						const int at = tr ? c * 6 + r : r * 6 + c;
						const long long q = to_fixed(x, 60 - ea6[r] - eb6[c], bad);
						if (dl) lds_add_i64(dl + at, q); else atomic_add_i64(dg + at, q);
					}
			}
		}
	}
	if (bad) atomic_add_i64(o.poison, 1);
	__syncthreads();
	for (int i = tid; i < SCHUR_CAP * 36; i += SCHUR_TILE)
	{
		const int k = skey[i / 36];
		if (k >= 0 && sval[i]) atomic_add_i64(o.S + (size_t)k * 36 + i % 36, sval[i]);
	}
	for (int i = tid; i < SCHUR_ECAP * 6; i += SCHUR_TILE)
	{
		const int k = ekey[i / 6];
		if (k >= 0)
		{
			if (evalv[i]) atomic_add_i64(o.Ehi + (size_t)k * 6 + i % 6, evalv[i]);
			if (evalv[SCHUR_ECAP * 6 + i]) atomic_add_i64(o.Elo + (size_t)k * 6 + i % 6, evalv[SCHUR_ECAP * 6 + i]);
		}
	}
}

// ---- K10a: y = S x on the upper-block storage, every stored block read ONCE --------------------------------
// A work-group owns SPT consecutive block rows.  Lane group g (8 lanes, lane r < 6 = scalar row r) takes blocks (p,q) of
// those rows: the row part B x_q goes to y_p and the mirrored part B^T x_p to y_q, both into an LDS window of y that
// covers the tile's rows and the SPW rows after them (S is a pose chain: q - p is small), flushed once with
// contiguous atomics.  Targets outside the window -- the columns of hub poses -- go through a small LDS table keyed
// by row.  Rows longer than SP_LONG blocks (the hub poses: up to a block per pose) are not walked by their own tile;
// instead every tile takes the hub blocks (h,q) whose COLUMN q it owns (their mirrored part lands in its window, their
// row part in the table under h).  So nothing is read twice, no wave scatters 8-byte atomics over 64 rows, and the
// index is just the upper block CSR plus the list of long rows.  (First version: a row-sorted index of both
// orientations -- every block read twice, one more sort per level.)   y must be zero on entry.
// dotw != null: dot[seg] += w . y (fused p.Ap).
#define SPT 16   /* block rows per work-group */
#define SPW 64   /* rows of the window after the tile */
#define SP_LONG 256
#define SP_FAR 64
#define SPMV_CACHED_BYTES ((size_t)96 << 20) /* a matrix up to this size is multiplied by k_spmv_gather (stays in L2 / Infinity Cache) */
__global__ void k_spmv_long_rows(int M, const int* __restrict__ rowptr, int* __restrict__ nlong, int* __restrict__ longrows)
{
	int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r < M && rowptr[r + 1] - rowptr[r] > SP_LONG) longrows[atomicAdd(nlong, 1)] = r;
}
__global__ void __launch_bounds__(256)
k_spmv(int M, const int* __restrict__ rowptr, const int* __restrict__ colidx, const int* __restrict__ nlong_p, const int* __restrict__ longrows,
       const double* __restrict__ S, const double* __restrict__ x, double* __restrict__ y, const unsigned char* __restrict__ fixed,
       const double* __restrict__ dotw, const int* __restrict__ pose_seg, double* __restrict__ dot, int dot_stride)
{
	__shared__ int pre[SPT + 1];               // prefix of the short rows' lengths
	__shared__ int rp[SPT + 1];
	__shared__ double ywin[(SPT + SPW) * 6];
	__shared__ int fkeys[SP_FAR];
	__shared__ double fvals[SP_FAR * 6];
	const int tid = threadIdx.x, g = tid >> 3, r = tid & 7, ng = blockDim.x >> 3;
	const int r0 = blockIdx.x * SPT, r1 = min(r0 + SPT, M), nr = r1 - r0;
	for (int i = tid; i < (SPT + SPW) * 6; i += blockDim.x) ywin[i] = 0.0;
	for (int i = tid; i < SP_FAR; i += blockDim.x) fkeys[i] = -1;
	for (int i = tid; i < SP_FAR * 6; i += blockDim.x) fvals[i] = 0.0;
	for (int i = tid; i <= nr; i += blockDim.x) rp[i] = rowptr[r0 + i];
	__syncthreads();
	if (tid == 0)
	{
		int acc = 0;
		for (int i = 0; i < nr; i++) { pre[i] = acc; const int len = rp[i + 1] - rp[i]; acc += len > SP_LONG ? 0 : len; }
		pre[nr] = acc;
	}
	__syncthreads();
	// target (row t, scalar r): window, table or global
	auto add = [&](int t, double v) {
		const int w = t - r0;
		if (w >= 0 && w < SPT + SPW) { lds_add_f64(&ywin[w * 6 + r], v); return; }
		const int sl = lds_slot(fkeys, SP_FAR, t);
		if (sl >= 0) { lds_add_f64(&fvals[sl * 6 + r], v); return; }
		// table full (a band wider than the window AND more far rows than slots): straight to memory, with its share of
		// the fused dot product
		if (fixed && fixed[(size_t)t * 6 + r]) return;
		atomic_add_f64(y + (size_t)t * 6 + r, v);
		if (dotw) atomic_add_f64(dot + (size_t)pose_seg[t] * dot_stride, dotw[(size_t)t * 6 + r] * v);
	};
	auto block = [&](int k, int p) {
		const int q = colidx[k];
		const double* blk = S + (size_t)k * 36;
		const double* xq = x + (size_t)q * 6;
		double sum = 0.0;
#pragma unroll
		for (int j = 0; j < 6; j++) sum = fma(blk[r * 6 + j], xq[j], sum);
		add(p, sum);
		if (q != p)
		{
			const double* xp = x + (size_t)p * 6;
			double t = 0.0;
#pragma unroll
			for (int j = 0; j < 6; j++) t = fma(blk[j * 6 + r], xp[j], t);
			add(q, t);
		}
	};
	// (1) the short rows of the tile
	const int nb = pre[nr];
	if (r < 6)
		for (int i = g; i < nb; i += ng)
		{
			int lo = 0, hi = nr - 1; // row of item i: last row with pre[row] <= i (rows of length 0 are skipped by the <=)
			while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pre[mid] <= i) lo = mid; else hi = mid - 1; }
			block(rp[lo] + (i - pre[lo]), r0 + lo);
		}
	// (2) the long rows: their blocks in the tile's columns.  One lane per long row finds where the tile's columns start
	// in it (all searches run side by side), then the lane groups take the blocks
	__shared__ int lstart[SP_FAR];
	const int nlong = *nlong_p;
	for (int l0 = 0; l0 < nlong; l0 += SP_FAR)
	{
		const int nl = min(SP_FAR, nlong - l0);
		__syncthreads();
		if (tid < nl)
		{
			const int h = longrows[l0 + tid];
			int lo = rowptr[h], hi = rowptr[h + 1]; // first block of row h with column >= r0
			// a hub row is (nearly) dense from its diagonal on: try the position a dense row would have first
			const int guess = lo + max(r0 - h, 0);
			if (guess < hi && colidx[guess] >= r0 && (guess == lo || colidx[guess - 1] < r0)) lo = guess;
			else
				while (lo < hi) { const int mid = (lo + hi) >> 1; if (colidx[mid] < r0) lo = mid + 1; else hi = mid; }
			lstart[tid] = lo;
		}
		__syncthreads();
		if (r < 6)
			for (int li = 0; li < nl; li++)
			{
				const int h = longrows[l0 + li], he = rowptr[h + 1];
				for (int k = lstart[li] + g; k < he && colidx[k] < r1; k += ng) block(k, h);
			}
	}
	__syncthreads();
	// (3) flush: the window (contiguous), then the far rows
	double w = 0.0;
	int seg = 0;
	bool any = false;
	for (int i = tid; i < (SPT + SPW) * 6; i += blockDim.x)
	{
		const int t = r0 + i / 6;
		const double v = ywin[i];
		if (t < M && v != 0.0 && !(fixed && fixed[(size_t)t * 6 + i % 6]))
		{
			atomic_add_f64(y + (size_t)t * 6 + i % 6, v);
			if (dotw)
			{
				const int sg = pose_seg[t];
				if (any && sg != seg) { atomic_add_f64(dot + (size_t)seg * dot_stride, w); w = 0.0; }
				seg = sg; any = true;
				w = fma(dotw[(size_t)t * 6 + i % 6], v, w);
			}
		}
	}
	for (int i = tid; i < SP_FAR * 6; i += blockDim.x)
	{
		const int t = fkeys[i / 6];
		const double v = fvals[i];
		if (t >= 0 && v != 0.0 && !(fixed && fixed[(size_t)t * 6 + i % 6]))
		{
			atomic_add_f64(y + (size_t)t * 6 + i % 6, v);
			if (dotw)
			{
				const int sg = pose_seg[t];
				if (any && sg != seg) { atomic_add_f64(dot + (size_t)seg * dot_stride, w); w = 0.0; }
				seg = sg; any = true;
				w = fma(dotw[(size_t)t * 6 + i % 6], v, w);
			}
		}
	}
	if (dotw) wave_scatter_add<1>(dot + (size_t)seg * dot_stride, &w, any);
}

// ---- K10a, cache-resident variant ------------------------------------------------------------------------------
// The Schur matrix of a tree level is at most a few tens of MB: it stays in L2 / Infinity Cache between the handful of
// products a level needs, so reading a block twice costs no HBM traffic, and with a path that revisits the band
// assumption of k_spmv (q - p small, a few hub rows) no longer holds -- at the top of the NC3500-like tree the windowed
// kernel spent 130 us per product walking ~100 "long" rows in every work-group.  Here both orientations of every block
// are listed once, sorted by the row they contribute to (structure only: built with the pattern, kept by the plan):
// entry = (target row << 32 | block << 1 | transposed), other[e] = the pose whose x it multiplies.  The product is a
// segmented sum over that list: 8 entries per 8-lane group (lane r < 6 = scalar row r), 256 entries per work-group,
// summed in an LDS window over the work-group's rows (at most 256: every row holds its diagonal block) and flushed with
// one atomic per touched scalar -- perfectly balanced whatever the row lengths are.  y must be zero on entry.
#define SPG_EPG 8
#define SPG_ENT (32 * SPG_EPG) /* entries per work-group of 256 lanes */
__global__ void k_spmv_gather_keys(int nnzb, const unsigned long long* __restrict__ upper_keys, unsigned long long* __restrict__ ent,
                                   int* __restrict__ oth)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= nnzb) return;
	const unsigned long long key = upper_keys[k];
	const unsigned p = (unsigned)(key >> 32), q = (unsigned)(key & 0xffffffffull);
	ent[k] = ((unsigned long long)p << 32) | ((unsigned)k << 1);
	oth[k] = (int)q;
	// the mirrored part of an off-diagonal block; diagonal blocks leave a hole that sorts to the end
	ent[(size_t)nnzb + k] = p != q ? (((unsigned long long)q << 32) | ((unsigned)k << 1) | 1u) : ~0ull;
	oth[(size_t)nnzb + k] = (int)p;
}
__global__ void __launch_bounds__(256)
k_spmv_gather(int M, int nent, const unsigned long long* __restrict__ ent, const int* __restrict__ oth, const double* __restrict__ S,
              const double* __restrict__ x, double* __restrict__ y, const unsigned char* __restrict__ fixed, const double* __restrict__ dotw,
              const int* __restrict__ pose_seg, double* __restrict__ dot, int dot_stride)
{
	__shared__ double ywin[SPG_ENT * 6];
	const int tid = threadIdx.x, g = tid >> 3, r = tid & 7;
	const int eb = blockIdx.x * SPG_ENT;
	const int row0 = (int)(ent[eb] >> 32); // first entry of the work-group: never a hole while eb < number of real entries
	for (int i = tid; i < SPG_ENT * 6; i += 256) ywin[i] = 0.0;
	__syncthreads();
	const int e0 = eb + g * SPG_EPG;
	if (r < 6 && e0 < nent && row0 >= 0)
	{
		unsigned long long key[SPG_EPG];
		int ot[SPG_EPG];
#pragma unroll
		for (int i = 0; i < SPG_EPG; i++)
		{
			const bool in = e0 + i < nent;
			key[i] = in ? ent[e0 + i] : ~0ull;
			ot[i] = in ? oth[e0 + i] : 0;
		}
		double sum[SPG_EPG];
#pragma unroll
		for (int i = 0; i < SPG_EPG; i++)
		{
			sum[i] = 0.0;
			if (key[i] == ~0ull) continue;
			const unsigned kk = (unsigned)(key[i] & 0xffffffffull);
			const double* blk = S + (size_t)(kk >> 1) * 36;
			const double* xo = x + (size_t)ot[i] * 6;
			double s = 0.0;
			if (kk & 1u)
			{
#pragma unroll
				for (int j = 0; j < 6; j++) s = fma(blk[j * 6 + r], xo[j], s);
			}
			else
			{
#pragma unroll
				for (int j = 0; j < 6; j++) s = fma(blk[r * 6 + j], xo[j], s);
			}
			sum[i] = s;
		}
		auto put = [&](int row, double v) {
			if (row - row0 < SPG_ENT) { lds_add_f64(&ywin[(row - row0) * 6 + r], v); return; }
			// a row without any block of its own between row0 and here (no diagonal block: not a Schur system, but stay correct)
			if (fixed && fixed[(size_t)row * 6 + r]) return;
			atomic_add_f64(y + (size_t)row * 6 + r, v);
			if (dotw) atomic_add_f64(dot + (size_t)pose_seg[row] * dot_stride, dotw[(size_t)row * 6 + r] * v);
		};
		int cur = -1;
		double acc = 0.0;
#pragma unroll
		for (int i = 0; i < SPG_EPG; i++)
		{
			if (key[i] == ~0ull) continue;
			const int row = (int)(key[i] >> 32);
			if (row != cur)
			{
				if (cur >= 0) put(cur, acc);
				cur = row; acc = 0.0;
			}
			acc += sum[i];
		}
		if (cur >= 0) put(cur, acc);
	}
	__syncthreads();
	double w = 0.0;
	int seg = 0;
	bool any = false;
	if (row0 >= 0)
		for (int i = tid; i < SPG_ENT * 6; i += 256)
		{
			const int t = row0 + i / 6;
			const double v = ywin[i];
			if (t < M && v != 0.0 && !(fixed && fixed[(size_t)t * 6 + i % 6]))
			{
				atomic_add_f64(y + (size_t)t * 6 + i % 6, v);
				if (dotw)
				{
					const int sg = pose_seg[t];
					if (any && sg != seg) { atomic_add_f64(dot + (size_t)seg * dot_stride, w); w = 0.0; }
					seg = sg; any = true;
					w = fma(dotw[(size_t)t * 6 + i % 6], v, w);
				}
			}
		}
	if (dotw) wave_scatter_add<1>(dot + (size_t)seg * dot_stride, &w, any);
}

// K11 (Imp.cpp:2980-3020); features of carried maps keep their values
#define BSUB_TILE 128 /* features per work-group */
__global__ void __launch_bounds__(256)
k_backsub(int NF, const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W,
          const double* __restrict__ IV, const double* __restrict__ eb, const double* __restrict__ xp,
          const int* __restrict__ feat_seg, const unsigned char* __restrict__ active, double* __restrict__ xf,
          const double* __restrict__ LY, const double* __restrict__ xhat)
{
	// one lane per W block (coalesced): W^T x_p, summed per feature through LDS; then x_f = V^-1 (eb - sum)
	__shared__ int sFp[BSUB_TILE + 1];
	__shared__ double sT[256 * 3];
	__shared__ double sS[BSUB_TILE * 3];
	const int f0 = blockIdx.x * BSUB_TILE, nft = min(BSUB_TILE, NF - f0);
	for (int i = threadIdx.x; i <= nft; i += blockDim.x) sFp[i] = fptr[f0 + i];
	for (int i = threadIdx.x; i < nft * 3; i += blockDim.x) sS[i] = 0.0;
	__syncthreads();
	tile_runs<3>(nft, sFp, sT,
		[&](int j, int, double* out) {
			double w[18];
			ld<18>(w, W + (size_t)j * 18);
			const double* a = xp + (size_t)photo[j] * 6;
			double a6[6];
			ld<6>(a6, a);
			if (xhat)
			{
				// (fused right-hand side: the step from the poses' estimates, see below)
				const double* h = xhat + (size_t)photo[j] * 6;
#pragma unroll
				for (int r = 0; r < 6; r++) a6[r] -= h[r];
			}
#pragma unroll
			for (int c = 0; c < 3; c++)
			{
				double sacc = 0.0;
#pragma unroll
				for (int r = 0; r < 6; r++) sacc = fma(w[3 * r + c], a6[r], sacc);
				out[c] = sacc;
			}
		},
		[&](int fl, int q, double sum, bool) { sS[fl * 3 + q] += sum; });
	for (int fl = threadIdx.x; fl < nft; fl += blockDim.x)
	{
		const int f = f0 + fl;
		if (active && !active[feat_seg[f]]) continue;
		if (xhat)
		{
			// fused right-hand side: eb as a whole was never formed (eb here is its V part; the W part is W^T x^_p, x^_p the poses'
			// estimates): x_f = V^-1 (eb + W^T x^_p - W^T x_p) = L (L^T eb - L^T s), s = sum W^T (x_p - x^_p) over the feature's run
			const double* l = LY + (size_t)f * 9;
			const double s0 = sS[fl * 3], s1 = sS[fl * 3 + 1], s2 = sS[fl * 3 + 2];
			const double d0 = l[6] - (l[0] * s0 + l[1] * s1 + l[3] * s2), d1 = l[7] - (l[2] * s1 + l[4] * s2),
			             d2 = l[8] - l[5] * s2;
			xf[(size_t)f * 3] = l[0] * d0; xf[(size_t)f * 3 + 1] = l[1] * d0 + l[2] * d1; xf[(size_t)f * 3 + 2] = l[3] * d0 + l[4] * d1 + l[5] * d2;
			continue;
		}
		const double* iv = IV + (size_t)f * 9;
		const double d[3] = { eb[(size_t)f * 3] - sS[fl * 3], eb[(size_t)f * 3 + 1] - sS[fl * 3 + 1], eb[(size_t)f * 3 + 2] - sS[fl * 3 + 2] };
		for (int r = 0; r < 3; r++) xf[(size_t)f * 3 + r] = iv[3 * r] * d[0] + iv[3 * r + 1] * d[1] + iv[3 * r + 2] * d[2];
	}
}

// -------------------------------------------------------------------------------------------------------------
__global__ void k_low_words(int n, const unsigned long long* __restrict__ keys, int* __restrict__ out)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = (int)(keys[i] & 0xffffffffull);
}

// the SpMV's index of a system whose sorted upper pattern exists (and, from lsfm_pattern.hip, its block CSR)
void build_spmv_index(lsfm_context* ctx, SchurSystem& sy, const unsigned long long* sorted_upper)
{
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	const int M = sy.M, cnt = sy.nnzb;
	if (!sy.rowptr)
	{
		sy.rowptr = sc.alloc<int>(M + 1);
		rowptr_from_keys(ctx, M, cnt, sorted_upper, sy.rowptr);
	}
	if (!sy.colidx)
	{
		sy.colidx = sc.alloc<int>(cnt + 1);
		if (cnt) hipLaunchKernelGGL(k_low_words, dim3((cnt + 255) / 256), dim3(256), 0, s, cnt, sorted_upper, sy.colidx);
	}
	// the only extra index: the rows with more than SP_LONG blocks (hub poses)
	int* nl = sc.alloc<int>(1);
	sy.longrows = sc.alloc<int>(M + 1);
	dev_zero(ctx, nl, sizeof(int));
	if (M) hipLaunchKernelGGL(k_spmv_long_rows, dim3((M + 255) / 256), dim3(256), 0, s, M, sy.rowptr, nl, sy.longrows);
	sy.d_nlong = nl;
	// a matrix that stays in the caches: the list of both orientations sorted by target row (k_spmv_gather)
	sy.gent = nullptr; sy.goth = nullptr;
	const int variant = ctx->pcg.spmv_variant;
	if (cnt && variant != 1 && (variant == 2 || (size_t)cnt * 288 <= SPMV_CACHED_BYTES))
	{
		unsigned long long* ent = sc.alloc<unsigned long long>((size_t)2 * cnt);
		int* oth = sc.alloc<int>((size_t)2 * cnt);
		hipLaunchKernelGGL(k_spmv_gather_keys, dim3((cnt + 255) / 256), dim3(256), 0, s, cnt, sorted_upper, ent, oth);
		// by target row only (the high word; the sort is stable and the product is a segmented sum over rows: the order inside a
		// row is free); the holes (all bits set) end up last
		int rb = 1;
		while ((1 << rb) <= M) rb++;
		dev_sort_pairs_u64(ctx, ent, oth, (size_t)2 * cnt, 32 + rb, 32);
		sy.gent = ent; sy.goth = oth;
	}
}

// K7: V^-1 of every feature (values: once per run)
void schur_vinv(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy)
{
	sy.IV = ctx->scratch.alloc<double>((size_t)io.NF * 9);
	sy.LY = ctx->scratch.alloc<double>((size_t)io.NF * 9);
	sy.ymax = ctx->scratch.alloc<double>((size_t)(io.NF + 255) / 256 + 1);
	sy.uu = nullptr;
	if (io.rhs) sy.uu = ctx->scratch.alloc<double>((size_t)io.NF * 6);
	if (io.NF) hipLaunchKernelGGL(k_vinv, dim3((io.NF + 255) / 256), dim3(256), 0, ctx->stream, io.NF, io.V, io.eb, sy.IV, sy.LY, sy.ymax, io.rhs ? *io.rhs : RhsFused(), sy.uu);
}

// Values of S and E: enqueued without a host synchronisation (the caller overlaps host work with K9); the K9 launch is
// bracketed by two events of the context's pool, whose time flush_times() adds to the run's statistics
void build_schur_values(lsfm_context* ctx, const SolveIO& io, SchurSystem& sy)
{
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	const int M = io.M, NF = io.NF, cnt = sy.nnzb;
	const unsigned long long* tab = sy.tab;
	const int* hval = sy.hval;
	const unsigned long long mask = sy.mask;
	const int ntiles = (NF + SCHUR_TILE - 1) / SCHUR_TILE;
	unsigned char* fb;
	// K9 adds in fixed point (order-independent, lsfm_device.hpp): the accumulators of W V^-1 W^T, the two limbs of -W V^-1 eb and the
	// poison word, back to back; S starts as U, E as the pose part of the right-hand side, k_schur_finish takes the sums off them
	const size_t nacc = 1 + (size_t)cnt * 36 + (size_t)M * 12;
	if (ctx->comm)
	{
		// feature-sharded run: the accumulators live in the caller's buffer; those of S (and the poison word ahead of them) are
		// summed over the ranks as INTEGERS -- exact, so every rank holds the same bits of S (U is replicated: every rank starts S
		// from it).  The right-hand side's limbs stay this rank's own -- their scale hangs on the rank's features (k_schur_scale: ey)
		// -- and E, this rank's part of it (its features' share of the pose part, rhs kernels of the join, U's on rank 0; its
		// features' -W V^-1 eb), is summed as doubles once k_schur_finish has put it together.
		ctx->comm->restart();
		sy.acc = ctx->comm->alloc<long long>(nacc);
		sy.E = ctx->comm->alloc<double>((size_t)M * 6);
		fill_async(s, sy.acc, 0, nacc * sizeof(long long));
		ZeroSpan zs(sc);
		sy.S = sc.alloc<double>((size_t)cnt * 36);
		fb = sc.alloc<unsigned char>(ntiles + 1);
		zs.zero(s);
	}
	else
	{
		ZeroSpan zs(sc);
		sy.S = sc.alloc<double>((size_t)cnt * 36);
		fb = sc.alloc<unsigned char>(ntiles + 1); // tiles the panel kernel hands to the per-feature kernel
		sy.acc = sc.alloc<long long>(nacc);
		zs.zero(s);
		sy.E = sc.alloc<double>((size_t)M * 6);
	}
	sy.sexp = sc.alloc<int>((size_t)M * 6 + 1);
	if (io.NU) hipLaunchKernelGGL(k_schur_u, dim3((io.NU + 255) / 256), dim3(256), 0, s, io.NU, io.U, io.Ui, io.Uj, tab, hval, mask, sy.S);
	hipLaunchKernelGGL(k_schur_scale, dim3((6 * M + 255) / 256 + 1), dim3(256), 0, s, M, sy.rowptr, sy.S, NF, NF ? (NF + 255) / 256 : 0, sy.ymax, io.d_fixed, sy.sexp, io.ea, sy.E);
	K9Out ko;
	ko.poison = sy.acc; ko.S = sy.acc + 1; ko.Ehi = ko.S + (size_t)cnt * 36; ko.Elo = ko.Ehi + (size_t)M * 6;
	ko.sexp = sy.sexp; ko.ey = sy.sexp + (size_t)M * 6;
	if (io.rhs) { ko.xpose = io.rhs->pose_src; ko.pside = io.rhs->pose_map_src; ko.uu = sy.uu; }
	if (NF)
	{
		// bracketed by HIP events on this stream: live duration of the K9 launch for the roofline line of bench.py
		hipEvent_t e2 = nullptr, e3 = nullptr;
		if (ctx->stats) { e2 = ctx->pool_event(); e3 = ctx->pool_event(); LSFM_REC_T(e2, s); }
		static_assert(LSFM_PM_TILE % SCHUR_TILE == 0, "a tile of the panel kernel must be whole tiles of the fallback kernel");
		// the per-tile slots of the panel variants: from the plan of the level, or worked out now (and left for the plan, if this
		// run makes one)
		bool fresh_lists = false;
		if (!sy.k9.ns)
		{
			fresh_lists = true;
			sy.k9.ns = sc.alloc<int>(ntiles + 1);
			sy.k9.pose = sc.alloc<int>((size_t)ntiles * 64 + 1);
			sy.k9.eslot = sc.alloc<unsigned char>((size_t)io.NW + 1);
			sy.k9.wlist = sc.alloc<int>((size_t)3 * ntiles + 1);
			sy.k9.wcnt = sc.alloc<int>(8);
			sy.k9_tiles = ntiles; sy.k9_NW = io.NW;
			launch_schur_slots(ctx, NF, io.fptr, io.photo, fb, sy.k9);
		}
		launch_schur_panel(ctx, NF, io.fptr, io.photo, io.W, sy.LY, tab, hval, mask, ko, fb, most_rows(io.seg_rows), sy.k9, fresh_lists);
		hipLaunchKernelGGL(k_schur_w, dim3(ntiles), dim3(SCHUR_TILE), 0, s, NF, io.fptr, io.photo, io.W, sy.IV, io.eb, tab, hval, mask, ko, fb, sy.LY);
		if (ctx->stats)
		{
			LSFM_REC_T(e3, s);
			ctx->defer_time(e2, e3, &ctx->stats->schur_ms);
			ctx->stats->schur_launches++;
			// every input once (W block + photo index; V^-1, eb, run pointer per feature), every output once (S, E)
			ctx->stats->schur_bytes += (double)io.NW * (144 + 4) + (double)io.NF * (72 + 24 + 4) + (double)sy.nnzb * 288 + (double)io.M * 48;
			// algorithmic flops of K9 = 144 NW + 108 (sum of squared run lengths + NW): the sum is taken on the device and read with
			// the run's record at the end of a tree run (lsfm_tree_run adds 108 x that)
			ctx->stats->schur_flops += (double)io.NW * (144.0 + 108.0);
			// (the W part of the right-hand sides, when K9 takes it along: eF += W^T x_p and eP += W x_f, 36 multiply-adds a block,
			// and the estimates they read -- until round 5 a pass of its own, k_join_rhs_w)
			if (io.rhs) { ctx->stats->schur_flops += (double)io.NW * 72.0; ctx->stats->schur_bytes += (double)io.NF * (48 + 24) + (double)io.M * 48; }
			// (on the side stream, behind the 16-slot variant and its event: a number for the run's statistics has no place in the
			// chain of the main stream -- 9 us per level; lsfm_tree_run waits for that stream before it reads the record, and the next
			// level for evR_done before it resets an arena: io.fptr lives in one)
			if (ctx->in_tree_run && ctx->d_run)
			{
				Fork side(ctx, ctx->stream2, evR_fork); // (the run pointers are final at this point of the main stream)
				hipLaunchKernelGGL(k_sum_run_squares, dim3(std::min((NF + 255) / 256, 512)), dim3(256), 0, ctx->stream, NF, io.fptr, &ctx->d_run->k2);
				side.done(evR_done);
			}
		}
	}
	if (ctx->comm) ctx->comm->allreduce(s, sy.acc, 1 + (size_t)cnt * 36, LSFM_DTYPE_I64);
	{
		const size_t n = (size_t)cnt * 36 + (size_t)M * 6;
		hipLaunchKernelGGL(k_schur_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cnt, M, sy.upper_keys, sy.acc, sy.sexp, sy.S, sy.E);
	}
	if (ctx->comm) ctx->comm->allreduce(s, sy.E, (size_t)M * 6, LSFM_DTYPE_F64);
	LSFM_CHECK_HIP(hipGetLastError());
}

void launch_spmv(lsfm_context* ctx, const SchurSystem& sy, const double* x, double* y, const unsigned char* fixed,
                 const double* dotw, const int* pose_seg, double* dot, int dot_stride)
{
	if (!sy.M) return;
	if (sy.gent)
	{
		// holes (the mirrored slots of the diagonal blocks) sort to the end: 2 nnzb - (diagonal blocks) real entries, at most 2 nnzb - 1
		const int nent = 2 * sy.nnzb;
		hipLaunchKernelGGL(k_spmv_gather, dim3((nent + SPG_ENT - 1) / SPG_ENT), dim3(256), 0, ctx->stream, sy.M, nent, sy.gent, sy.goth, sy.S, x, y, fixed,
		                   dotw, pose_seg, dot, dot_stride);
		return;
	}
	hipLaunchKernelGGL(k_spmv, dim3((sy.M + SPT - 1) / SPT), dim3(256), 0, ctx->stream, sy.M, sy.rowptr, sy.colidx, sy.d_nlong, sy.longrows, sy.S, x, y,
	                   fixed, dotw, pose_seg, dot, dot_stride);
}

// algorithmic bytes of one SpMV on the upper-block storage: blocks + column indices + row pointers + x and y
double spmv_bytes(const SchurSystem& sy) { return (double)sy.nnzb * (288 + 4) + 4.0 * (sy.M + 1) + 2.0 * 48 * sy.M; }

void launch_backsub(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const double* x)
{
	if (io.NF)
		hipLaunchKernelGGL(k_backsub, dim3((io.NF + BSUB_TILE - 1) / BSUB_TILE), dim3(256), 0, ctx->stream, io.NF, io.fptr, io.photo, io.W, sy.IV, io.eb, x,
		                   io.d_feat_seg, io.d_seg_active, io.x_feat, sy.LY, io.rhs ? io.rhs->pose_src : (const double*)nullptr);
}

// the two feature-side pieces of the solve on their own, from and to host arrays (C ABI: lsfm_inverse_v / lsfm_solve_features)
int inverse_v(lsfm_context* ctx, double* V, int n)
{
	ctx->ensure_arenas((size_t)n * 400 + ((size_t)64 << 20));
	ctx->arena[0].reset(); ctx->scratch.reset();
	double* dV = ctx->arena[0].alloc<double>((size_t)n * 9);
	double* dIV = ctx->arena[0].alloc<double>((size_t)n * 9);
	h2d(ctx, dV, V, (size_t)n * 9 * sizeof(double));
	if (n)
	{
		double* LY = ctx->scratch.alloc<double>((size_t)n * 9);
		double* eb = ctx->scratch.alloc<double>((size_t)n * 3);
		dev_zero(ctx, eb, (size_t)n * 3 * sizeof(double));
		hipLaunchKernelGGL(k_vinv, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, dV, eb, dIV, LY, (double*)nullptr, RhsFused(), (double*)nullptr);
		LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	}
	d2h(ctx, V, dIV, (size_t)n * 9 * sizeof(double));
	return LSFM_OK;
}
// C ABI: lsfm_selftest_vinv -- k_vinv alone with both of its records back; skip doubles in front of every device array
int vinv_selftest(lsfm_context* ctx, const double* V, const double* eb, int n, int skip, double* IV, double* LY)
{
	ctx->ensure_arenas((size_t)n * 400 + ((size_t)64 << 20));
	ctx->arena[0].reset(); ctx->scratch.reset();
	Arena& ar = ctx->arena[0];
	double* dV = ar.alloc<double>((size_t)n * 9 + skip) + skip;
	double* deb = ar.alloc<double>((size_t)n * 3 + skip) + skip;
	double* dIV = ar.alloc<double>((size_t)n * 9 + skip) + skip;
	double* dLY = ar.alloc<double>((size_t)n * 9 + skip) + skip;
	if (!n) return LSFM_OK;
	h2d(ctx, dV, V, (size_t)n * 9 * sizeof(double));
	h2d(ctx, deb, eb, (size_t)n * 3 * sizeof(double));
	hipLaunchKernelGGL(k_vinv, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, dV, deb, dIV, dLY, (double*)nullptr, RhsFused(), (double*)nullptr);
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	d2h(ctx, IV, dIV, (size_t)n * 9 * sizeof(double));
	d2h(ctx, LY, dLY, (size_t)n * 9 * sizeof(double));
	return LSFM_OK;
}
int solve_features(lsfm_context* ctx, const double* W, const double* IV, const double* eb, const double* dpa, double* dpb, int m, int n, const int* mapCor,
                   const int* photo)
{
	std::vector<int> fptr((size_t)n + 1, 0);
	for (int f = 0; f < n; f++)
	{
		if (mapCor[f] < 0) LSFM_FAIL(LSFM_ERR_ARG, "negative block count of a feature");
		fptr[f + 1] = fptr[f] + mapCor[f];
	}
	const int nW = fptr[n];
	for (int j = 0; j < nW; j++) if (photo[j] < 0 || photo[j] >= m) LSFM_FAIL(LSFM_ERR_ARG, "photo index out of range");
	ctx->ensure_arenas((size_t)nW * 200 + (size_t)n * 300 + (size_t)m * 100 + ((size_t)64 << 20));
	ctx->arena[0].reset(); ctx->scratch.reset();
	Arena& ar = ctx->arena[0];
	double* dW = ar.alloc<double>((size_t)nW * 18); int* dph = ar.alloc<int>(nW); int* dfp = ar.alloc<int>((size_t)n + 1);
	double* dIV = ar.alloc<double>((size_t)n * 9); double* deb = ar.alloc<double>((size_t)n * 3);
	double* dxp = ar.alloc<double>((size_t)m * 6); double* dxf = ar.alloc<double>((size_t)n * 3);
	h2d(ctx, dW, W, (size_t)nW * 18 * sizeof(double)); h2d(ctx, dph, photo, (size_t)nW * sizeof(int));
	h2d(ctx, dfp, fptr.data(), ((size_t)n + 1) * sizeof(int)); h2d(ctx, dIV, IV, (size_t)n * 9 * sizeof(double));
	h2d(ctx, deb, eb, (size_t)n * 3 * sizeof(double)); h2d(ctx, dxp, dpa, (size_t)m * 6 * sizeof(double));
	if (n)
		hipLaunchKernelGGL(k_backsub, dim3((n + BSUB_TILE - 1) / BSUB_TILE), dim3(256), 0, ctx->stream, n, dfp, dph, dW, dIV, deb, dxp,
		                   (const int*)nullptr, (const unsigned char*)nullptr, dxf, (const double*)nullptr, (const double*)nullptr);
	d2h(ctx, dpb, dxf, (size_t)n * 3 * sizeof(double));
	return LSFM_OK;
}

// y = S x for an externally supplied symmetric block matrix (upper block CSR): measurement entry of the C ABI
int spmv_external(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const double* x, double* y, int reps,
                  double* avg_ms, double* bytes)
{
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	size_t mk = sc.mark();
	const int nnzb = rowptr[m];
	SchurSystem sy;
	sy.M = m; sy.nnzb = nnzb;
	std::vector<unsigned long long> keys(nnzb);
	for (int p = 0; p < m; p++)
		for (int k = rowptr[p]; k < rowptr[p + 1]; k++) keys[k] = ((unsigned long long)(unsigned)p << 32) | (unsigned)colidx[k];
	unsigned long long* dk = sc.alloc<unsigned long long>(nnzb + 1);
	sy.S = sc.alloc<double>((size_t)nnzb * 36);
	double* dx = sc.alloc<double>((size_t)m * 6);
	double* dy = sc.alloc<double>((size_t)m * 6);
	h2d(ctx, dk, keys.data(), (size_t)nnzb * sizeof(unsigned long long));
	h2d(ctx, sy.S, val, (size_t)nnzb * 36 * sizeof(double));
	h2d(ctx, dx, x, (size_t)m * 6 * sizeof(double));
	build_spmv_index(ctx, sy, dk);
	float total = 0;
	hipEvent_t e0 = ctx->pool_event(), e1 = ctx->pool_event();
	for (int k = 0; k < reps + 2; k++)
	{
		dev_zero(ctx, dy, (size_t)m * 6 * sizeof(double));
		LSFM_CHECK_HIP(hipEventRecord(e0, s));
		launch_spmv(ctx, sy, dx, dy, nullptr, nullptr, nullptr, nullptr, 1);
		LSFM_CHECK_HIP(hipEventRecord(e1, s));
		LSFM_CHECK_HIP(hipEventSynchronize(e1));
		float t = 0;
		LSFM_CHECK_HIP(hipEventElapsedTime(&t, e0, e1));
		if (k >= 2) total += t;
	}
	d2h(ctx, y, dy, (size_t)m * 6 * sizeof(double));
	if (avg_ms) *avg_ms = reps > 0 ? total / reps : 0;
	if (bytes) *bytes = spmv_bytes(sy);
	sc.release(mk);
	return 0;
}

} // namespace lsfm
