// Marginalising features out of a map (C ABI: lsfm_map_marginalise, lsfm_tree_export_reduced_*).  No reference counterpart: the
// reference keeps every feature of every local map to the end.
//
// With the features split into kept (k) and dropped (d), the marginal of I = [U W; W^T V] over the dropped ones is
//     U' = U - sum_{f in d} W_f V_f^-1 W_f^T,   W' = W_k,   V' = V_k
// -- V is block diagonal, so the fill lands in U alone and the result is a map again.  The sum is the one a tree level takes over ALL
// its features when it reduces its camera system, so the level's own pieces take it, chained as cov_front (lsfm_cov.hip) chains them:
// schur_vinv -> build_schur_pattern -> build_schur_values (K9: fixed-point sums, order independent) on a SolveIO that holds U and the
// dropped features only.  S = U - sums is then U', its sorted key list (row << 32 | col) the coordinates.
// K9 wants the W runs of its features back to back, so the dropped runs are made contiguous first:
//   k_marg_flags + two scans   new index of every kept feature and the start of its W run; a dropped feature's follow by
//                              subtraction (f - kpos[f], fptr[f] - kwpos[f]): one scan pair serves both sides
//   k_marg_index / _photo      run pointers and poses of the dropped features (what the pattern needs: index arrays alone)
//   k_marg_w                   THE pass over W: every 144-byte block is read once and written to exactly one of two places -- a kept
//                              block to the output (with its pose and renumbered feature), a dropped block to K9's input; order
//                              inside a run is preserved.  One lane per block, as k_slice_w (lsfm_batch.hip) and k_gn_coalesce<18>
//   k_marg_features            per feature: V, estimate, label and run pointer of a kept one to the output, V of a dropped one to
//                              k_vinv's input
//   k_marg_emit                U' / Ui / Uj from S and its keys, consecutive lanes on consecutive numbers
// A dropped V that is not positive definite leaves a NaN in k_vinv's factor (LY); its tile then goes to K9's per-feature kernel, which
// forms a finite -- and wrong -- sum from the indefinite inverse without tripping its bound, so the poison word alone would miss it:
// k_marg_status reads both, the caller reads one int.  A kept feature's V is never inverted.
// A pose scalar whose diagonal entry is zero (the gauge scalars of a Mono map) gets scale 0 from k_schur_scale and nothing is added
// to it: its row and column stay exactly zero, no gauge mask is passed (d_fixed = nullptr).
#include <algorithm>
#include <cstring>
#include <vector>

#include "lsfm_device.hpp"
#include "lsfm_marg.hpp"
#include "lsfm_system.hpp"

namespace lsfm {

namespace {

// keep[] sorted ascending: is id in it?
__global__ void k_marg_flag_keep(int NF, const int* __restrict__ feat_id, const int* __restrict__ keep, int nkeep, int* __restrict__ drop)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f > NF) return;
	if (f == NF) { drop[f] = 0; return; }
	const int id = feat_id[f];
	int lo = 0, hi = nkeep; // first entry >= id
	while (lo < hi) { const int mid = (lo + hi) >> 1; if (keep[mid] < id) lo = mid + 1; else hi = mid; }
	drop[f] = (lo < nkeep && keep[lo] == id) ? 0 : 1;
}
// what the two scans run over: kept flag and kept run length per feature (entry NF: 0)
__global__ void k_marg_flags(int NF, const int* __restrict__ drop, const int* __restrict__ fptr, int* __restrict__ kf, int* __restrict__ kl)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f > NF) return;
	const bool kept = f < NF && !drop[f];
	kf[f] = kept ? 1 : 0;
	kl[f] = kept ? fptr[f + 1] - fptr[f] : 0;
}
__global__ void k_marg_counts(int NF, const int* __restrict__ kpos, const int* __restrict__ kwpos, int* __restrict__ cnt)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) { cnt[0] = kpos[NF]; cnt[1] = kwpos[NF]; }
}
// run pointers of the dropped features (entry NF closes the last run: NF - kpos[NF] = dropped features, fptr[NF] - kwpos[NF] = their blocks)
__global__ void k_marg_index(int NF, const int* __restrict__ drop, const int* __restrict__ fptr, const int* __restrict__ kpos, const int* __restrict__ kwpos,
                             int* __restrict__ dfp)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f > NF) return;
	if (f == NF || drop[f]) dfp[f - kpos[f]] = fptr[f] - kwpos[f];
}
// poses of the dropped blocks: block j of dropped feature f lands at (fptr[f] - kwpos[f]) + (j - fptr[f]) = j - kwpos[f]
__global__ void k_marg_photo(int NW, const int* __restrict__ feature, const int* __restrict__ drop, const int* __restrict__ kwpos, const int* __restrict__ photo,
                             int* __restrict__ dph)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NW) return;
	const int f = feature[j];
	if (drop[f]) dph[j - kwpos[f]] = photo[j];
}
// the partition pass over W: one lane per block, the block as 18 doubles (oW == null: the kept blocks stay where they are)
__global__ void __launch_bounds__(256)
k_marg_w(int NW, const int* __restrict__ feature, const int* __restrict__ fptr, const int* __restrict__ drop, const int* __restrict__ kpos,
         const int* __restrict__ kwpos, const double* __restrict__ W, const int* __restrict__ photo, double* __restrict__ dW, double* __restrict__ oW,
         int* __restrict__ ophoto, int* __restrict__ ofeature)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NW) return;
	const int f = feature[j];
	const bool dr = drop[f] != 0;
	if (!dr && !oW) return;
	double w[18];
	ld<18>(w, W + (size_t)j * 18);
	if (dr) { st<18>(dW + (size_t)(j - kwpos[f]) * 18, w); return; }
	const int d = kwpos[f] + (j - fptr[f]);
	st<18>(oW + (size_t)d * 18, w);
	ophoto[d] = photo[j];
	if (ofeature) ofeature[d] = kpos[f];
}
__global__ void k_marg_features(int NF, const int* __restrict__ drop, const int* __restrict__ kpos, const int* __restrict__ kwpos, const double* __restrict__ V,
                                const double* __restrict__ feat, const int* __restrict__ feat_id, double* __restrict__ dV, MargKept o)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f > NF) return;
	if (f == NF) { if (o.fptr) o.fptr[kpos[NF]] = kwpos[NF]; return; }
	double v[9];
	ld<9>(v, V + (size_t)f * 9);
	if (drop[f]) { st<9>(dV + (size_t)(f - kpos[f]) * 9, v); return; }
	if (!o.V) return;
	const int p = kpos[f];
	st<9>(o.V + (size_t)p * 9, v);
	for (int c = 0; c < 3; c++) o.feat[(size_t)p * 3 + c] = feat[(size_t)f * 3 + c];
	o.feat_id[p] = feat_id[f];
	o.fptr[p] = kwpos[f];
}
// != 0: a dropped V without a Cholesky factor (k_vinv marks it with a NaN), or K9's poison word
__global__ void k_marg_status(int ND, const double* __restrict__ LY, const long long* __restrict__ acc, int* __restrict__ err)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f == 0 && acc[0] != 0) atomicExch(err, 2);
	if (f < ND) { const double l = LY[(size_t)f * 9]; if (!(l == l)) atomicExch(err, 1); }
}
__global__ void __launch_bounds__(256)
k_marg_emit(int nnzb, const unsigned long long* __restrict__ keys, const double* __restrict__ S, double* __restrict__ oU, int* __restrict__ oUi, int* __restrict__ oUj)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)nnzb * 36) return;
	oU[i] = S[i];
	if (i % 36 == 0)
	{
		const unsigned long long key = keys[i / 36];
		oUi[i / 36] = (int)(key >> 32); oUj[i / 36] = (int)(key & 0xffffffffull);
	}
}

inline dim3 grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

} // namespace

void marg_flags_from_keep(lsfm_context* ctx, int NF, const int* feat_id, const int* keep_sorted, int nkeep, int* drop)
{
	hipLaunchKernelGGL(k_marg_flag_keep, grid((size_t)NF + 1), dim3(256), 0, ctx->stream, NF, feat_id, keep_sorted, nkeep, drop);
}

void marg_structure(lsfm_context* ctx, Arena& ar, const MargView& in, const int* drop, int nkeep, int nWkeep, MargWork& w)
{
	hipStream_t s = ctx->stream;
	const int M = in.M, NF = in.NF, NW = in.NW;
	w.in = in; w.drop = drop;
	int* kf = ar.alloc<int>((size_t)NF + 2);
	int* kl = ar.alloc<int>((size_t)NF + 2);
	w.kpos = ar.alloc<int>((size_t)NF + 2);
	w.kwpos = ar.alloc<int>((size_t)NF + 2);
	hipLaunchKernelGGL(k_marg_flags, grid((size_t)NF + 1), dim3(256), 0, s, NF, drop, in.fptr, kf, kl);
	dev_exclusive_scan(ctx, kf, w.kpos, NF);
	dev_exclusive_scan(ctx, kl, w.kwpos, NF);
	if (nkeep < 0 || nWkeep < 0)
	{
		int* cnt = ar.alloc<int>(2);
		hipLaunchKernelGGL(k_marg_counts, dim3(1), dim3(64), 0, s, NF, w.kpos, w.kwpos, cnt);
		int h[2] = { 0, 0 };
		d2h_ints(ctx, cnt, h, 2);
		nkeep = h[0]; nWkeep = h[1];
	}
	if (nkeep < 0 || nkeep > NF || nWkeep < 0 || nWkeep > NW) LSFM_FAIL(LSFM_ERR_INTERNAL, "kept counts out of range");
	w.nkeep = nkeep; w.nWkeep = nWkeep; w.ndrop = NF - nkeep; w.nWdrop = NW - nWkeep;
	w.dfp = ar.alloc<int>((size_t)w.ndrop + 1);
	w.dph = ar.alloc<int>((size_t)w.nWdrop + 1);
	hipLaunchKernelGGL(k_marg_index, grid((size_t)NF + 1), dim3(256), 0, s, NF, drop, in.fptr, w.kpos, w.kwpos, w.dfp);
	if (NW) hipLaunchKernelGGL(k_marg_photo, grid(NW), dim3(256), 0, s, NW, in.feature, drop, w.kwpos, in.photo, w.dph);
	// K9's input: U and the dropped features; the right-hand side is not used (zeros), one system, no gauge mask
	int* seg = ar.alloc<int>((size_t)M + w.ndrop + 1);
	double* ea = ar.alloc<double>((size_t)M * 6);
	double* eb = ar.alloc<double>((size_t)w.ndrop * 3 + 1);
	dev_zero(ctx, seg, ((size_t)M + w.ndrop + 1) * sizeof(int));
	dev_zero(ctx, ea, (size_t)M * 6 * sizeof(double));
	dev_zero(ctx, eb, ((size_t)w.ndrop * 3 + 1) * sizeof(double));
	SolveIO& io = w.io;
	io = SolveIO();
	io.M = M; io.NF = w.ndrop; io.NU = in.NU; io.NW = w.nWdrop; io.nseg = 1;
	io.d_pose_seg = seg; io.d_feat_seg = seg + M;
	io.U = in.U; io.Ui = in.Ui; io.Uj = in.Uj; io.photo = w.dph; io.fptr = w.dfp; io.ea = ea; io.eb = eb;
	io.seg_rows.assign(1, M);
	w.sy = SchurSystem();
	build_schur_pattern(ctx, io, w.sy);
	LSFM_CHECK_HIP(hipGetLastError());
}

void marg_values(lsfm_context* ctx, Arena& ar, MargWork& w, const MargKept& kept, double* oU, int* oUi, int* oUj, int* d_err, hipEvent_t* ev)
{
	hipStream_t s = ctx->stream;
	const MargView& in = w.in;
	double* dW = ar.alloc<double>((size_t)w.nWdrop * 18 + 1);
	double* dV = ar.alloc<double>((size_t)w.ndrop * 9 + 1);
	if (in.NW)
		hipLaunchKernelGGL(k_marg_w, grid(in.NW), dim3(256), 0, s, in.NW, in.feature, in.fptr, w.drop, w.kpos, w.kwpos, in.W, in.photo, dW, kept.W, kept.photo,
		                   kept.feature);
	if (ev) LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	hipLaunchKernelGGL(k_marg_features, grid((size_t)in.NF + 1), dim3(256), 0, s, in.NF, w.drop, w.kpos, w.kwpos, in.V, in.feat, in.feat_id, dV, kept);
	w.io.W = dW; w.io.V = dV;
	schur_vinv(ctx, w.io, w.sy);
	if (ev) LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	build_schur_values(ctx, w.io, w.sy);
	if (ev) LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	hipLaunchKernelGGL(k_marg_status, grid((size_t)w.ndrop + 1), dim3(256), 0, s, w.ndrop, w.sy.LY, w.sy.acc, d_err);
	const int nnzb = w.sy.nnzb;
	if (nnzb) hipLaunchKernelGGL(k_marg_emit, grid((size_t)nnzb * 36), dim3(256), 0, s, nnzb, w.sy.upper_keys, w.sy.S, oU, oUi, oUj);
	LSFM_CHECK_HIP(hipGetLastError());
}

int map_marginalise(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out, double* times)
{
	const int m = map->m, n = map->n;
	// ---- arguments (host) ----
	const HostSystem h = host_system_of(*map, true);
	const std::vector<int> fptr = system_fptr(h);
	std::vector<int> hdrop(n + 1, 0);
	int nkeep = 0, nWkeep = 0;
	for (int f = 0; f < n; f++)
	{
		hdrop[f] = drop[f] ? 1 : 0;
		if (!drop[f]) { nkeep++; nWkeep += fptr[f + 1] - fptr[f]; }
	}
	// ---- upload (lsfm_system.hip) ----
	SolveIO up;
	MargView in;
	system_upload(ctx, h, SYS_VALUES | SYS_FEATURE, fptr, nullptr, up, &in.feature);
	Arena& ar = ctx->arena[0];
	hipStream_t s = ctx->stream;
	int* ddrop = ar.alloc<int>(n + 1);
	h2d(ctx, ddrop, hdrop.data(), (n + 1) * sizeof(int));
	in.M = m; in.NF = n; in.NU = up.NU; in.NW = up.NW;
	in.U = up.U; in.Ui = up.Ui; in.Uj = up.Uj; in.W = up.W; in.photo = up.photo; in.fptr = up.fptr; in.V = up.V;
	hipEvent_t ev[5]; // start | partition pass | V^-1 | K9 values | downloaded
	for (int k = 0; k < 5; k++) ev[k] = ctx->pool_event();
	LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	// ---- reduce: the kept blocks are compacted on the host below, only the dropped ones move on the device ----
	MargWork w;
	marg_structure(ctx, ar, in, ddrop, nkeep, nWkeep, w);
	const int nnzb = w.sy.nnzb;
	double* oU = ar.alloc<double>((size_t)nnzb * 36); int* oUi = ar.alloc<int>(nnzb); int* oUj = ar.alloc<int>(nnzb);
	int* d_err = ar.alloc<int>(1);
	dev_zero(ctx, d_err, sizeof(int));
	marg_values(ctx, ar, w, MargKept(), oU, oUi, oUj, d_err, ev + 1);
	int err = 0;
	d2h(ctx, &err, d_err, sizeof(int));
	if (err) LSFM_FAIL(LSFM_ERR_NOT_SPD, "the V block of a feature to be marginalised out is not positive definite");
	// ---- the map (library-allocated) ----
	MapOut G;
	map_new(G.g, map, m, nkeep, nnzb, nWkeep, map->pose_origin != nullptr);
	lsfm_map& g = G.g;
	if (map->pose_origin) memcpy(g.pose_origin, map->pose_origin, (size_t)m * sizeof(int));
	d2h(ctx, g.U, oU, (size_t)nnzb * 36 * sizeof(double));
	d2h(ctx, g.Ui, oUi, (size_t)nnzb * sizeof(int));
	d2h(ctx, g.Uj, oUj, (size_t)nnzb * sizeof(int));
	LSFM_CHECK_HIP(hipEventRecord(ev[4], s));
	LSFM_CHECK_HIP(hipEventSynchronize(ev[4]));
	if (times)
	{
		times[0] = event_ms(ev[0], ev[2]);
		times[1] = event_ms(ev[2], ev[3]);
		times[2] = event_ms(ev[3], ev[4]);
	}
	memcpy(g.stno, map->stno, (size_t)6 * m * sizeof(int));
	memcpy(g.stVal, map->stVal, (size_t)6 * m * sizeof(double));
	int p = 0, q = 0;
	for (int f = 0; f < n; f++)
	{
		if (drop[f]) continue;
		const int len = fptr[f + 1] - fptr[f];
		memcpy(g.stno + (size_t)6 * m + (size_t)3 * p, map->stno + (size_t)6 * m + (size_t)3 * f, 3 * sizeof(int));
		memcpy(g.stVal + (size_t)6 * m + (size_t)3 * p, map->stVal + (size_t)6 * m + (size_t)3 * f, 3 * sizeof(double));
		memcpy(g.V + (size_t)9 * p, map->V + (size_t)9 * f, 9 * sizeof(double));
		memcpy(g.W + (size_t)18 * q, map->W + (size_t)18 * fptr[f], (size_t)len * 18 * sizeof(double));
		memcpy(g.photo + q, map->photo + fptr[f], (size_t)len * sizeof(int));
		for (int a = 0; a < len; a++) g.feature[q + a] = p;
		g.FBlock[p] = q;
		p++; q += len;
	}
	G.give(out);
	return LSFM_OK;
}

void marg_export_reduced(lsfm_context* ctx, const DevBatch& b, bool mono, Arena& ar, const int* keep_ids, int nkeep, void* dst, size_t cap, size_t* bytes,
                         double* times)
{
	if (b.W_alias) LSFM_FAIL(LSFM_ERR_INTERNAL, "cannot pack a batch whose W blocks are aliased");
	// work space: `ar`, and the scratch arena above what is there
	struct Scratch { Arena& a; size_t mk; ~Scratch() { a.release(mk); } } hold{ ctx->scratch, ctx->scratch.mark() };
	ar.reset();
	hipStream_t s = ctx->stream;
	std::vector<int> keep(keep_ids, keep_ids + nkeep);
	std::sort(keep.begin(), keep.end());
	int* d_keep = ar.alloc<int>((size_t)nkeep + 1);
	h2d(ctx, d_keep, keep.data(), (size_t)nkeep * sizeof(int));
	hipEvent_t ev[6]; // start | structure | partition pass | gather + V^-1 | K9 values | emitted
	if (times) { for (int k = 0; k < 6; k++) ev[k] = ctx->pool_event(); LSFM_CHECK_HIP(hipEventRecord(ev[0], s)); }
	int* drop = ar.alloc<int>((size_t)b.NF + 2);
	marg_flags_from_keep(ctx, b.NF, b.feat_id, d_keep, nkeep, drop);
	MargView in; // (a single map: its indices are local already)
	in.M = b.M; in.NF = b.NF; in.NU = b.NU; in.NW = b.NW;
	in.U = b.U; in.Ui = b.Ui; in.Uj = b.Uj; in.W = b.W; in.photo = b.photo; in.feature = b.feature; in.fptr = b.fptr; in.V = b.V;
	in.feat = b.feat; in.feat_id = b.feat_id;
	MargWork w;
	marg_structure(ctx, ar, in, drop, -1, -1, w);
	PackHeader h;
	memset(&h, 0, sizeof h);
	h.magic = LSFM_PACK_MAGIC; h.version = 1; h.mono = mono;
	h.m = b.M; h.n = w.nkeep; h.nU = w.sy.nnzb; h.nW = w.nWkeep;
	h.Ref = b.Ref[0]; h.FRef = b.FRef[0]; h.ScaP = b.ScaP[0]; h.Fix = b.Fix[0]; h.Sign = b.Sign[0]; h.FScaP = b.FScaP[0]; h.FFix = b.FFix[0];
	const size_t total = pack_layout(h);
	if (bytes) *bytes = total;
	if (!dst) return;
	if (total > cap) LSFM_FAIL(LSFM_ERR_ARG, "export buffer too small: " + std::to_string(total) + " bytes needed");
	char* d = static_cast<char*>(dst);
	h2d(ctx, d, &h, sizeof h);
	auto cp = [&](int slot, const void* src, size_t n) {
		if (n) LSFM_CHECK_HIP(hipMemcpyAsync(d + h.off[slot], src, n, hipMemcpyDeviceToDevice, s));
	};
	cp(0, b.pose, (size_t)h.m * 48); cp(5, b.pose_id, (size_t)h.m * 4); cp(6, b.pose_origin, (size_t)h.m * 4);
	MargKept kept;
	kept.feat = reinterpret_cast<double*>(d + h.off[1]); kept.W = reinterpret_cast<double*>(d + h.off[3]); kept.V = reinterpret_cast<double*>(d + h.off[4]);
	kept.feat_id = reinterpret_cast<int*>(d + h.off[7]); kept.photo = reinterpret_cast<int*>(d + h.off[10]); kept.fptr = reinterpret_cast<int*>(d + h.off[11]);
	int* d_err = ar.alloc<int>(1);
	dev_zero(ctx, d_err, sizeof(int));
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	marg_values(ctx, ar, w, kept, reinterpret_cast<double*>(d + h.off[2]), reinterpret_cast<int*>(d + h.off[8]), reinterpret_cast<int*>(d + h.off[9]), d_err,
	            times ? ev + 2 : nullptr);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[5], s));
	int err = 0;
	d2h(ctx, &err, d_err, sizeof(int)); // (synchronises: the caller hands dst to another library / stream next)
	if (times)
		for (int k = 0; k < 5; k++) times[k] = event_ms(ev[k], ev[k + 1]);
	if (err) LSFM_FAIL(LSFM_ERR_NOT_SPD, "the V block of a feature to be marginalised out is not positive definite");
}

} // namespace lsfm
