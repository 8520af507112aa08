// C ABI (include/lsfm.h): argument checks and the error boundary of every entry point.  The work is elsewhere -- the tree scheduler in
// lsfm_tree.hip, a system from host arrays in lsfm_system.hip, each stage in its own file.
#include <climits>
#include <cmath>
#include <cstring>

#include "lsfm_internal.hpp"
#include "lsfm_marg.hpp"
#include "lsfm_solve.hpp"
#include "lsfm_system.hpp"
#include "lsfm_tree.hpp"

using namespace lsfm;

namespace {

template <class F> int guarded(lsfm_context* ctx, F&& f)
{
	if (!ctx) return LSFM_ERR_ARG;
	struct Reset { // per-call state that must not outlive the call (sinks of deferred timings point into the caller's frame)
		lsfm_context* c;
		~Reset() { c->timed.clear(); c->ev_next = 0; c->plan = nullptr; }
	} reset{ ctx };
	try
	{
		if (hipSetDevice(ctx->device) != hipSuccess) return LSFM_ERR_NO_DEVICE;
		return f();
	}
	catch (const Error& e)
	{
		ctx->last_error = e.msg;
		fprintf(stderr, "liblsfm_hip: %s\n", e.msg.c_str());
		(void)hipGetLastError();
		ctx->quiesce_side_streams(); // (the next call resets arenas that work left on stream2 or stream3 may still be reading)
		return e.code;
	}
	catch (const std::exception& e)
	{
		ctx->last_error = e.what();
		ctx->quiesce_side_streams();
		return LSFM_ERR_INTERNAL;
	}
}

// the result of a finished run, still where the run left it (single_map: the run went up to the root)
void require_result(const lsfm_context* ctx, const lsfm_tree* t, bool single_map = true)
{
	if (!t->done || (single_map && t->level.B != 1)) LSFM_FAIL(LSFM_ERR_ARG, "tree has not been run");
	if (t->generation != ctx->generation)
		LSFM_FAIL(LSFM_ERR_ARG, "the result of this tree was overwritten by a later call on the same context (it lives in the context's arenas): "
		                        "download a tree before the context is used for anything else, or run it again");
}

// the headers of N packed maps (device buffers)
std::vector<PackHeader> pack_headers(lsfm_context* ctx, const void* const* packed, int N)
{
	std::vector<PackHeader> hdr(N);
	for (int k = 0; k < N; k++)
	{
		if (!packed[k]) LSFM_FAIL(LSFM_ERR_ARG, "null packed map");
		LSFM_CHECK_HIP(hipMemcpyAsync(&hdr[k], packed[k], sizeof(PackHeader), hipMemcpyDeviceToHost, ctx->stream));
	}
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	return hdr;
}

size_t input_bytes(const lsfm_map* maps, int N)
{
	size_t nw = 0, nf = 0, nu = 0, m = 0;
	for (int k = 0; k < N; k++) { nw += maps[k].nW; nf += maps[k].n; nu += maps[k].nU; m += maps[k].m; }
	return m * 64 + nf * 120 + nu * 300 + nw * 156 + (size_t)N * 16 + ((size_t)1 << 20);
}

} // namespace

extern "C" {

int lsfm_tree_upload(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, lsfm_tree** out)
{
	if (!out || !maps || N <= 0) return LSFM_ERR_ARG;
	*out = nullptr;
	return guarded(ctx, [&]() {
		ctx->ensure_arenas(estimate_arena(maps, N, tree_levels(N)), true);
		lsfm_tree* t = new lsfm_tree();
		t->mono = mono != 0; t->N = N; t->slot = 0;
		ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
		try
		{
			t->input_arena.init(input_bytes(maps, N));
			const double t0 = now_ms();
			batch_upload(ctx, t->input_arena, maps, N, t->mono, t->input);
			LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
			t->upload_ms = now_ms() - t0;
		}
		catch (...) { t->input_arena.destroy(); delete t; throw; }
		*out = t;
		return LSFM_OK;
	});
}

int lsfm_tree_run(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* stats)
{
	if (!t) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return tree_run(ctx, t, stats); });
}

int lsfm_tree_set_plans(lsfm_tree* t, int on)
{
	if (!t) return LSFM_ERR_ARG;
	t->use_plans = on != 0;
	if (!on) t->plans.clear();
	return LSFM_OK;
}

int lsfm_tree_download(lsfm_context* ctx, lsfm_tree* t, lsfm_map* out)
{
	if (!t || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		batch_download_map(ctx, t->level, 0, t->mono, out);
		return LSFM_OK;
	});
}

int lsfm_tree_download_state(lsfm_context* ctx, lsfm_tree* t, int* m, int* n, int* stno, double* stVal, size_t cap)
{
	if (!t || !m || !n) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		const DevBatch& b = t->level;
		*m = b.M; *n = b.NF;
		if (!stno && !stVal) return LSFM_OK;
		const size_t r = (size_t)6 * b.M + (size_t)3 * b.NF;
		if (cap < r) LSFM_FAIL(LSFM_ERR_ARG, "state arrays too small");
		if (stVal)
		{
			d2h(ctx, stVal, b.pose, (size_t)b.M * 6 * sizeof(double));
			d2h(ctx, stVal + (size_t)6 * b.M, b.feat, (size_t)b.NF * 3 * sizeof(double));
		}
		if (stno)
		{
			std::vector<int> pid(b.M), fid(b.NF);
			d2h(ctx, pid.data(), b.pose_id, (size_t)b.M * sizeof(int));
			d2h(ctx, fid.data(), b.feat_id, (size_t)b.NF * sizeof(int));
			for (int i = 0; i < b.M; i++) for (int c = 0; c < 6; c++) stno[6 * (size_t)i + c] = -pid[i];
			for (int i = 0; i < b.NF; i++) for (int c = 0; c < 3; c++) stno[6 * (size_t)b.M + 3 * (size_t)i + c] = fid[i];
		}
		return LSFM_OK;
	});
}

size_t lsfm_tree_export_size(lsfm_context* ctx, lsfm_tree* t)
{
	if (!ctx || !t || !t->done || t->level.B != 1 || t->generation != ctx->generation) return 0;
	PackHeader h;
	memset(&h, 0, sizeof h);
	const DevBatch& b = t->level;
	h.m = b.M; h.n = b.NF; h.nU = b.NU; h.nW = b.NW;
	return pack_layout(h);
}

int lsfm_tree_export_dev(lsfm_context* ctx, lsfm_tree* t, void* dst, size_t cap)
{
	if (!t || !dst) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		batch_pack_map(ctx, t->level, 0, t->mono, dst, cap);
		LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream)); // the caller hands dst to another library / stream next
		return LSFM_OK;
	});
}

static_assert(sizeof(PackHeader) == LSFM_PACK_HEADER_BYTES, "include/lsfm.h documents the header size");
size_t lsfm_packed_size(const void* host_header)
{
	if (!host_header) return 0;
	PackHeader h;
	memcpy(&h, host_header, sizeof h);
	if (h.magic != LSFM_PACK_MAGIC || h.version != 1 || h.m < 0 || h.n < 0 || h.nU < 0 || h.nW < 0) return 0;
	// the offsets an unpack follows are the ones the sizes imply, never just what the buffer says
	PackHeader c = h;
	if (pack_layout(c) != h.total) return 0;
	for (int i = 0; i < 12; i++) if (c.off[i] != h.off[i]) return 0;
	return (size_t)h.total;
}

int lsfm_tree_upload_dev(lsfm_context* ctx, const void* const* packed, int N, int mono, lsfm_tree** out)
{
	if (!out || !packed || N <= 0) return LSFM_ERR_ARG;
	*out = nullptr;
	return guarded(ctx, [&]() {
		const std::vector<PackHeader> hdr = pack_headers(ctx, packed, N);
		size_t nw = 0, nf = 0, nu = 0, m = 0, bytes = 0;
		for (int k = 0; k < N; k++)
		{
			if (lsfm_packed_size(&hdr[k]) == 0) LSFM_FAIL(LSFM_ERR_ARG, "buffer " + std::to_string(k) + " is not a packed map");
			if ((hdr[k].mono != 0) != (mono != 0)) LSFM_FAIL(LSFM_ERR_ARG, "packed map of the other camera type");
			nw += hdr[k].nW; nf += hdr[k].n; nu += hdr[k].nU; m += hdr[k].m; bytes += hdr[k].total;
		}
		ctx->ensure_arenas(estimate_arena(nw, nf, nu, m, tree_levels(N)));
		lsfm_tree* t = new lsfm_tree();
		t->mono = mono != 0; t->N = N; t->slot = 0;
		ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
		try
		{
			t->input_arena.init(bytes + (m + nf + nw) * 8 + (size_t)N * 4096 + ((size_t)1 << 20));
			batch_unpack_maps(ctx, t->input_arena, packed, hdr.data(), N, t->mono, t->input);
			t->digest = batch_structure_digest(ctx, t->input);
			LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
		}
		catch (...) { t->input_arena.destroy(); delete t; throw; }
		*out = t;
		return LSFM_OK;
	});
}

int lsfm_tree_reload_dev(lsfm_context* ctx, lsfm_tree* t, const void* const* packed, int N)
{
	if (!t || !packed || N != t->N) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		const std::vector<PackHeader> hdr = pack_headers(ctx, packed, N);
		const DevBatch& b = t->input;
		for (int k = 0; k < N; k++)
		{
			const PackHeader& h = hdr[k];
			if (lsfm_packed_size(&h) == 0 || (h.mono != 0) != t->mono || h.m != b.pose_off[k + 1] - b.pose_off[k] || h.n != b.feat_off[k + 1] - b.feat_off[k] ||
			    h.nU != b.u_off[k + 1] - b.u_off[k] || h.nW != b.w_off[k + 1] - b.w_off[k])
				LSFM_FAIL(LSFM_ERR_ARG, "packed map " + std::to_string(k) + " does not have the sizes of the tree's resident map (reload keeps the structure)");
		}
		ctx->generation++;
		t->done = false;
		t->input_arena.reset(); // same sizes, same order: every array lands where it was
		batch_unpack_maps(ctx, t->input_arena, packed, hdr.data(), N, t->mono, t->input);
		ctx->scratch.reset();
		const unsigned long long dg = batch_structure_digest(ctx, t->input);
		if (dg != t->digest)
		{
			// same sizes, other labels / index arrays: everything the plans hold (S pattern, K9 slots, join offsets) is void
			t->plans.clear();
			t->digest = dg;
		}
		LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
		return LSFM_OK;
	});
}

int lsfm_tree_set_comm(lsfm_tree* t, int rank, int world, lsfm_allreduce_fn fn, void* user, void* dev_buf, size_t dev_bytes)
{
	if (!t) return LSFM_ERR_ARG;
	if (!fn) { t->comm = Comm(); return LSFM_OK; }
	if (world < 1 || rank < 0 || rank >= world || !dev_buf || dev_bytes < 4096) return LSFM_ERR_ARG;
	if (t->comm.rank != rank || t->comm.world != world) t->plans.clear();
	t->comm.rank = rank; t->comm.world = world; t->comm.fn = fn; t->comm.user = user;
	t->comm.buf = static_cast<char*>(dev_buf); t->comm.cap = dev_bytes; t->comm.restart(); t->comm.broken = false;
	return LSFM_OK;
}

int lsfm_tree_set_comm_blocks(lsfm_tree* t, int block_maps)
{
	if (!t || block_maps < 0 || (block_maps & (block_maps - 1))) return LSFM_ERR_ARG; // (blocks of the reference's pairing are 2^k local maps)
	if (t->comm.block_maps != block_maps) t->plans.clear(); // (the plans hold the ownership of every factorisation)
	t->comm.block_maps = block_maps;
	return LSFM_OK;
}

int lsfm_tree_export_slice_sizes(lsfm_context* ctx, lsfm_tree* t, int nslices, size_t* sizes)
{
	if (!t || !sizes || nslices <= 0) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		if (t->slice_n != nslices)
		{
			// how many features and W blocks every slice holds: structure -- counted once, kept for the later runs of the tree
			batch_slice_counts(ctx, t->level, nslices, t->slice_nf, t->slice_nw);
			t->slice_n = nslices;
		}
		const DevBatch& b = t->level;
		for (int g = 0; g < nslices; g++)
		{
			PackHeader h;
			memset(&h, 0, sizeof h);
			h.m = b.M; h.n = t->slice_nf[g]; h.nU = b.NU; h.nW = t->slice_nw[g];
			sizes[g] = pack_layout(h);
		}
		return LSFM_OK;
	});
}

int lsfm_tree_export_slice_dev(lsfm_context* ctx, lsfm_tree* t, int nslices, int slice, void* dst, size_t cap)
{
	if (!t || !dst || nslices <= 0 || slice < 0 || slice >= nslices) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		if (t->slice_n != nslices) LSFM_FAIL(LSFM_ERR_ARG, "call lsfm_tree_export_slice_sizes with the same number of slices first");
		const size_t mk = ctx->scratch.mark();
		batch_pack_slice(ctx, t->level, t->mono, nslices, slice, t->slice_nf[slice], t->slice_nw[slice], dst, cap);
		LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream)); // the caller hands dst to another library / stream next
		ctx->scratch.release(mk);
		return LSFM_OK;
	});
}

// (an arena the result does not live in)
static Arena& reduced_work_arena(lsfm_context* ctx, const lsfm_tree* t) { return ctx->arena[t->slot < 0 ? 0 : (t->slot + 1) % 3]; }

int lsfm_tree_export_reduced_size(lsfm_context* ctx, lsfm_tree* t, const int* keep_ids, int nkeep, size_t* bytes)
{
	if (!t || !bytes || nkeep < 0 || (nkeep > 0 && !keep_ids)) return LSFM_ERR_ARG;
	*bytes = 0;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		marg_export_reduced(ctx, t->level, t->mono, reduced_work_arena(ctx, t), keep_ids, nkeep, nullptr, 0, bytes, nullptr);
		return LSFM_OK;
	});
}

int lsfm_tree_export_reduced_dev_timed(lsfm_context* ctx, lsfm_tree* t, const int* keep_ids, int nkeep, void* dst, size_t cap, double* times)
{
	if (!t || !dst || nkeep < 0 || (nkeep > 0 && !keep_ids)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t);
		marg_export_reduced(ctx, t->level, t->mono, reduced_work_arena(ctx, t), keep_ids, nkeep, dst, cap, nullptr, times);
		return LSFM_OK;
	});
}

int lsfm_tree_export_reduced_dev(lsfm_context* ctx, lsfm_tree* t, const int* keep_ids, int nkeep, void* dst, size_t cap)
{
	return lsfm_tree_export_reduced_dev_timed(ctx, t, keep_ids, nkeep, dst, cap, nullptr);
}

int lsfm_tree_set_stop_level(lsfm_tree* t, int levels)
{
	if (!t || levels < 0) return LSFM_ERR_ARG;
	t->stop_level = levels;
	return LSFM_OK;
}

int lsfm_tree_node_count(lsfm_context* ctx, lsfm_tree* t)
{
	if (!ctx || !t || !t->done || t->generation != ctx->generation) return 0;
	return t->level.B;
}

int lsfm_tree_download_node(lsfm_context* ctx, lsfm_tree* t, int k, lsfm_map* out)
{
	if (!t || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		require_result(ctx, t, false);
		if (k < 0 || k >= t->level.B) LSFM_FAIL(LSFM_ERR_ARG, "node index out of range");
		batch_download_map(ctx, t->level, k, t->mono, out);
		return LSFM_OK;
	});
}

int lsfm_tree_set_final_reanchor(lsfm_tree* t, int on)
{
	if (!t) return LSFM_ERR_ARG;
	t->final_reanchor = on != 0;
	return LSFM_OK;
}

void lsfm_tree_free(lsfm_context* ctx, lsfm_tree* t)
{
	if (!t) return;
	if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
	t->input_arena.destroy();
	delete t;
}

int lsfm_divide_conquer(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, lsfm_map* out, lsfm_stats* stats)
{
	lsfm_tree* t = nullptr;
	int rc = lsfm_tree_upload(ctx, maps, N, mono, &t);
	if (rc) return rc;
	t->use_plans = false; // one run, then the tree is gone: nothing to record for a next one
	int rrc = lsfm_tree_run(ctx, t, stats);
	if (rrc < 0) { lsfm_tree_free(ctx, t); return rrc; }
	rc = lsfm_tree_download(ctx, t, out);
	lsfm_tree_free(ctx, t);
	return rc ? rc : rrc;
}

static int transform_one(lsfm_context* ctx, const lsfm_map* in, int Ref, int ScaP, int Fix, bool mono, lsfm_map* out)
{
	if (!in || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		ctx->ensure_arenas(estimate_arena(in, 1, 1));
		ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
		DevBatch X, Y;
		batch_upload(ctx, ctx->arena[0], in, 1, mono, X);
		std::vector<int> tref(1, Ref), tscap(1, ScaP), tfix(1, Fix);
		transform_batch(ctx, ctx->arena[1], X, tref, tscap, tfix, mono, Y);
		batch_download_map(ctx, Y, 0, mono, out);
		return LSFM_OK;
	});
}

int lsfm_transform_stereo(lsfm_context* ctx, const lsfm_map* in, int Ref, lsfm_map* out) { return transform_one(ctx, in, Ref, 0, 0, false, out); }
int lsfm_transform_mono(lsfm_context* ctx, const lsfm_map* in, int Ref, int ScaP, int Fix, lsfm_map* out)
{
	return transform_one(ctx, in, Ref, ScaP, Fix, true, out);
}

static int join_one(lsfm_context* ctx, const lsfm_map* End, const lsfm_map* Cur, bool mono, lsfm_map* joint, double* eP_out, double* eF_out)
{
	if (!End || !Cur || !joint) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		lsfm_map two[2] = { *End, *Cur };
		ctx->ensure_arenas(estimate_arena(two, 2, 1));
		ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
		DevBatch X, Y;
		batch_upload(ctx, ctx->arena[0], two, 2, mono, X);
		lsfm_stats st;
		memset(&st, 0, sizeof st);
		{
			struct Sink { lsfm_context* c; Sink(lsfm_context* x, lsfm_stats* s) : c(x) { c->stats = s; } ~Sink() { c->stats = nullptr; } } sink(ctx, &st);
			(mono ? join_batch_mono : join_batch_stereo)(ctx, ctx->arena[1], X, Y, eP_out, eF_out, 0);
		}
		batch_download_map(ctx, Y, 0, mono, joint);
		return st.not_converged ? LSFM_NOT_CONVERGED : LSFM_OK;
	});
}

int lsfm_join_stereo(lsfm_context* ctx, const lsfm_map* End, const lsfm_map* Cur, lsfm_map* joint, double* eP_out, double* eF_out)
{
	return join_one(ctx, End, Cur, false, joint, eP_out, eF_out);
}
int lsfm_join_mono(lsfm_context* ctx, const lsfm_map* End, const lsfm_map* Cur, lsfm_map* joint, double* eP_out, double* eF_out)
{
	return join_one(ctx, End, Cur, true, joint, eP_out, eF_out);
}

// raw-pointer solver with the reference's argument list (Imp.h:209 / 223); fixed_blk / fixed_scalar < 0: Stereo
static int solve_raw(lsfm_context* ctx, double* stVal, const double* eb, const double* ea, const double* U, const double* W,
                     const double* V, const int* Ui, const int* Uj, const int* photo, const int* feature, int m, int n, int nU,
                     int nW, const double* x0, int fixed_blk, int fixed_scalar)
{
	if (!stVal || m <= 0 || n < 0 || nU < 0 || nW < 0) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		HostSystem h;
		h.m = m; h.n = n; h.nU = nU; h.nW = nW;
		h.Ui = Ui; h.Uj = Uj; h.photo = photo; h.feature = feature;
		h.U = U; h.W = W; h.V = V; h.ea = ea; h.eb = eb; h.x0 = x0;
		const std::vector<int> fptr = system_fptr(h);
		const bool gauge = fixed_blk >= 0 || fixed_scalar >= 0;
		const std::vector<unsigned char> fx = gauge ? gauge_mask(m, fixed_blk, fixed_scalar) : std::vector<unsigned char>();
		SolveIO io;
		// (the one-launch dense path walks a level by the ranges of its systems)
		system_upload(ctx, h, SYS_VALUES | SYS_RHS | SYS_X | (small_level_strips(ctx, m) ? SYS_OFFSETS : 0u), fptr, gauge ? &fx : nullptr, io);
		const int rc = solve_batch(ctx, io).not_converged;
		d2h(ctx, stVal, io.x_pose, (size_t)m * 6 * sizeof(double));
		d2h(ctx, stVal + 6 * m, io.x_feat, (size_t)n * 3 * sizeof(double));
		return rc ? LSFM_NOT_CONVERGED : LSFM_OK;
	});
}

int lsfm_solve_stereo(lsfm_context* ctx, double* stVal, const double* eb, const double* ea, const double* U, const double* W,
                      const double* V, const int* Ui, const int* Uj, const int* photo, const int* feature, int m, int n, int nU,
                      int nW, const double* x0)
{
	return solve_raw(ctx, stVal, eb, ea, U, W, V, Ui, Uj, photo, feature, m, n, nU, nW, x0, -1, -1);
}

// Imp.cpp:6756-7041: the 6 scalars of block `Ref` (= scalars ScaP..ScaP+5, the call site passes ScaP = 6*Ref) and scalar
// `Fix` are removed from the system, the solution is 0 there, and finally stVal[Fix] = Sign (Imp.cpp:7026)
int lsfm_solve_mono(lsfm_context* ctx, double* stVal, const double* eb, const double* ea, const double* U, const double* W,
                    const double* V, const int* Ui, const int* Uj, const int* photo, const int* feature, int m, int n, int nU,
                    int nW, int Ref, int ScaP, int Fix, int Sign, int FixBlk, const double* x0)
{
	(void)FixBlk;
	if (ScaP != 6 * Ref || Ref < 0 || Ref >= m || Fix < 0 || Fix >= 6 * m) return LSFM_ERR_ARG;
	int rc = solve_raw(ctx, stVal, eb, ea, U, W, V, Ui, Uj, photo, feature, m, n, nU, nW, x0, Ref, Fix);
	if (rc >= 0) stVal[Fix] = Sign;
	return rc;
}

int lsfm_gn_polish(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, double* obj, double* gnorm, int* halvings)
{
	if (!maps || N <= 0 || !x || iters < 0 || !obj || !gnorm || (type != 0 && type != 1)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return gn_polish(ctx, maps, N, type == 1, x, iters, 0, 1.0, obj, gnorm, halvings, nullptr, nullptr); });
}

int lsfm_gn_polish_robust(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, int kind, double c, double* obj,
                          double* gnorm, int* halvings, double* chi2, double* weight)
{
	if (!maps || N <= 0 || !x || iters < 0 || !obj || !gnorm || (type != 0 && type != 1) || kind < 0 || kind > 2 || !(c > 0.0) || !std::isfinite(c))
		return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return gn_polish(ctx, maps, N, type == 1, x, iters, kind, c, obj, gnorm, halvings, chi2, weight); });
}

int lsfm_map_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, double* chi2, int* dof)
{
	if (!maps || N <= 0 || !x || !chi2 || (type != 0 && type != 1)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_chi2(ctx, maps, N, type == 1, x, chi2, dof); });
}

int lsfm_map_feature_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, double* fchi2, double* pose_chi2)
{
	if (!maps || N <= 0 || !x || !fchi2 || (type != 0 && type != 1)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_feature_chi2(ctx, maps, N, type == 1, x, fchi2, pose_chi2); });
}

int lsfm_gn_polish_robust_features(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, int kind, double c, double* obj,
                                   double* gnorm, int* halvings, double* fchi2, double* fweight)
{
	if (!maps || N <= 0 || !x || iters < 0 || !obj || !gnorm || (type != 0 && type != 1) || kind < 0 || kind > 2 || !(c > 0.0) || !std::isfinite(c))
		return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return gn_polish_features(ctx, maps, N, type == 1, x, iters, kind, c, obj, gnorm, halvings, fchi2, fweight); });
}

int lsfm_gn_linearise_timed(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight, lsfm_map* out, double* obj,
                            double* b, double* times, int* counts)
{
	if (!maps || N <= 0 || !x || !out || (type != 0 && type != 1)) return LSFM_ERR_ARG;
	if (weight)
		for (int k = 0; k < N; k++)
			if (!std::isfinite(weight[k]) || weight[k] < 0.0)
				return guarded(ctx, [&]() -> int { LSFM_FAIL(LSFM_ERR_ARG, "gn linearise: weight " + std::to_string(k + 1) + " is negative or not finite"); });
	return guarded(ctx, [&]() { return gn_linearise(ctx, maps, N, type == 1, x, weight, nullptr, out, obj, b, times, counts); });
}

int lsfm_gn_linearise_features_timed(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight,
                                     const double* fweight, lsfm_map* out, double* obj, double* b, double* times, int* counts)
{
	if (!maps || N <= 0 || !x || !out || !fweight || (type != 0 && type != 1)) return LSFM_ERR_ARG;
	if (weight)
		for (int k = 0; k < N; k++)
			if (!std::isfinite(weight[k]) || weight[k] < 0.0)
				return guarded(ctx, [&]() -> int { LSFM_FAIL(LSFM_ERR_ARG, "gn linearise: weight " + std::to_string(k + 1) + " is negative or not finite"); });
	// (a map with a negative size is refused by the upload, before a weight of it would be read)
	size_t q = 0;
	for (int k = 0; k < N && maps[k].n >= 0; q += (size_t)maps[k].n, k++)
		for (int f = 0; f < maps[k].n; f++)
			if (!(fweight[q + f] >= 0.0 && fweight[q + f] <= 1.0))
				return guarded(ctx, [&]() -> int {
					LSFM_FAIL(LSFM_ERR_ARG, "gn linearise: the weight of feature " + std::to_string(f + 1) + " of local map " + std::to_string(k + 1) + " is not in [0, 1]");
				});
	return guarded(ctx, [&]() { return gn_linearise(ctx, maps, N, type == 1, x, weight, fweight, out, obj, b, times, counts); });
}

int lsfm_gn_linearise_features(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight, const double* fweight,
                               lsfm_map* out, double* obj, double* b)
{
	return lsfm_gn_linearise_features_timed(ctx, maps, N, type, x, weight, fweight, out, obj, b, nullptr, nullptr);
}

int lsfm_gn_linearise(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight, lsfm_map* out, double* obj,
                      double* b)
{
	return lsfm_gn_linearise_timed(ctx, maps, N, type, x, weight, out, obj, b, nullptr, nullptr);
}

// What the single-map calls ask of their map before anything runs: mono is 0 or 1, at least one pose, no negative size, no null array
// that its sizes say is read, the labels (stno) of a Mono map -- its gauge is found by them -- and what `need` adds.
enum MapNeeds : unsigned {
	MAP_STVAL = 1u << 0, // the estimates
	MAP_STNO  = 1u << 1, // the labels whatever mono is
};
static bool map_ok(const lsfm_map* map, int mono, unsigned need)
{
	if (!map || (mono != 0 && mono != 1) || map->m <= 0 || map->n < 0 || map->nU < 0 || map->nW < 0) return false;
	if ((map->nU && (!map->U || !map->Ui || !map->Uj)) || (map->nW && (!map->W || !map->photo || !map->feature)) || (map->n && !map->V)) return false;
	return !(((mono || (need & MAP_STNO)) && !map->stno) || ((need & MAP_STVAL) && !map->stVal));
}

int lsfm_map_covariance_timed(lsfm_context* ctx, const lsfm_map* map, int mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb,
                              double* times)
{
	if (!map_ok(map, mono, 0) || (pair_cov && (cap_blocks < 0 || !nnzb))) return LSFM_ERR_ARG;
	int cnt = 0;
	const int rc = guarded(ctx, [&]() { return map_covariance(ctx, map, mono == 1, pose_cov, feat_cov, pair_cov, cap_blocks, &cnt, times); });
	if (nnzb) *nnzb = cnt;
	return rc;
}

int lsfm_map_covariance(lsfm_context* ctx, const lsfm_map* map, int mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb)
{
	return lsfm_map_covariance_timed(ctx, map, mono, pose_cov, feat_cov, pair_cov, cap_blocks, nnzb, nullptr);
}

int lsfm_map_marginalise_timed(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out, double* times)
{
	if (!map || !drop || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_marginalise(ctx, map, drop, out, times); });
}

int lsfm_map_marginalise(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out)
{
	return lsfm_map_marginalise_timed(ctx, map, drop, out, nullptr);
}

int lsfm_map_marginalise_poses_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat, lsfm_map* out,
                                     double* times, int* info)
{
	if (!map_ok(map, mono, MAP_STNO | MAP_STVAL) || !keep_pose || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_marginalise_poses(ctx, map, mono == 1, keep_pose, drop_feat, out, times, info); });
}

int lsfm_map_marginalise_poses(lsfm_context* ctx, const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat, lsfm_map* out)
{
	return lsfm_map_marginalise_poses_timed(ctx, map, mono, keep_pose, drop_feat, out, nullptr, nullptr);
}

int lsfm_map_covariance_columns_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* poses, int k, double* pose_cols, double* feat_cols,
                                      double* joint, int* steps, double* last_corr, double* times)
{
	if (!map_ok(map, mono, 0) || !poses || k < 1 || (!pose_cols && !feat_cols && !joint)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_covariance_columns(ctx, map, mono == 1, poses, k, pose_cols, feat_cols, joint, steps, last_corr, times); });
}

int lsfm_map_covariance_columns(lsfm_context* ctx, const lsfm_map* map, int mono, const int* poses, int k, double* pose_cols, double* feat_cols, double* joint,
                                int* steps, double* last_corr)
{
	return lsfm_map_covariance_columns_timed(ctx, map, mono, poses, k, pose_cols, feat_cols, joint, steps, last_corr, nullptr);
}

int lsfm_map_covariance_feature_columns_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* feats, int k, double* pose_cols, double* feat_cols,
                                              double* joint, int* steps, double* last_corr, double* times)
{
	if (!map_ok(map, mono, 0) || !feats || k < 1 || (!pose_cols && !feat_cols && !joint)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_covariance_feature_columns(ctx, map, mono == 1, feats, k, pose_cols, feat_cols, joint, steps, last_corr, times); });
}

int lsfm_map_covariance_feature_columns(lsfm_context* ctx, const lsfm_map* map, int mono, const int* feats, int k, double* pose_cols, double* feat_cols,
                                        double* joint, int* steps, double* last_corr)
{
	return lsfm_map_covariance_feature_columns_timed(ctx, map, mono, feats, k, pose_cols, feat_cols, joint, steps, last_corr, nullptr);
}

int lsfm_map_feature_pair_gate_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps,
                                     double* last_corr, double* times)
{
	if (!map_ok(map, mono, MAP_STVAL) || !pairs || K < 1 || (!d2 && !cov_diff)) return LSFM_ERR_ARG; // (the estimates: the gate's x_f - x_g)
	return guarded(ctx, [&]() { return map_feature_pair_gate(ctx, map, mono == 1, pairs, K, d2, cov_diff, steps, last_corr, times); });
}

int lsfm_map_feature_pair_gate(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps,
                               double* last_corr)
{
	return lsfm_map_feature_pair_gate_timed(ctx, map, mono, pairs, K, d2, cov_diff, steps, last_corr, nullptr);
}

int lsfm_map_feature_pair_joint_gate_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, const int* order, double tau,
                                           int* status, double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps,
                                           double* last_corr, double* times)
{
	if (steps) *steps = 0;
	if (!map_ok(map, mono, MAP_STVAL) || !pairs || K < 1 || !status || !delta || !accepted || !implied || !D2) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		return map_feature_pair_joint_gate(ctx, map, mono == 1, pairs, K, order, tau, status, delta, d2, joint_C, accepted, implied, D2, steps, last_corr, times);
	});
}

int lsfm_map_feature_pair_joint_gate(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, const int* order, double tau, int* status,
                                     double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps, double* last_corr)
{
	return lsfm_map_feature_pair_joint_gate_timed(ctx, map, mono, pairs, K, order, tau, status, delta, d2, joint_C, accepted, implied, D2, steps, last_corr, nullptr);
}

int lsfm_selftest_pair_select(lsfm_context* ctx, int K, const double* Cm, const double* d, const int* ends, const int* order, double tau, int* status,
                              double* delta, double* D2, int* accepted, int* implied)
{
	if (K < 1 || !Cm || !d || !ends || !status || !delta || !D2 || !accepted || !implied) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return pair_select_selftest(ctx, K, Cm, d, ends, order, tau, status, delta, D2, accepted, implied); });
}

int lsfm_map_merge_features_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof, int* rep,
                                  int* steps, double* last_corr, double* times)
{
	if (steps) *steps = 0;
	if (!map_ok(map, mono, MAP_STNO | MAP_STVAL) || !pairs || K < 1 || !out) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return map_merge_features(ctx, map, mono == 1, pairs, K, out, d2, dof, rep, steps, last_corr, times); });
}

int lsfm_map_merge_features(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof, int* rep,
                            int* steps, double* last_corr)
{
	return lsfm_map_merge_features_timed(ctx, map, mono, pairs, K, out, d2, dof, rep, steps, last_corr, nullptr);
}

int lsfm_map_feature_pair_candidates_timed(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs,
                                           double* dist2, double* q, long long cap, long long* count, double* times, long long* info)
{
	// (neither U, W nor V is read: the map needs its sizes and, where it has features, its estimates)
	if (!map || map->m < 0 || map->n < 0 || (map->n && !map->stVal) || !count) return LSFM_ERR_ARG;
	long long cnt = 0; // (set even where the call throws: a cap that is too small)
	const int rc = guarded(ctx, [&]() { return map_feature_pair_candidates(ctx, map, feat_cov, radius, tau, pairs, dist2, q, cap, &cnt, times, info); });
	*count = cnt;
	return rc;
}

int lsfm_map_feature_pair_candidates(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs, double* dist2,
                                     double* q, long long cap, long long* count)
{
	return lsfm_map_feature_pair_candidates_timed(ctx, map, feat_cov, radius, tau, pairs, dist2, q, cap, count, nullptr, nullptr);
}

int lsfm_inverse_v(lsfm_context* ctx, double* V, int m, int n)
{
	(void)m;
	if (n < 0 || (n && !V)) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return inverse_v(ctx, V, n); });
}

int lsfm_selftest_vinv(lsfm_context* ctx, const double* V, const double* eb, int n, int skip, double* IV, double* LY)
{
	if (n < 0 || skip < 0 || skip > 1 || (n && (!V || !eb || !IV || !LY))) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return vinv_selftest(ctx, V, eb, n, skip, IV, LY); });
}

int lsfm_solve_features(lsfm_context* ctx, const double* W, const double* IV, const double* ea, const double* eb, const double* dpa, double* dpb,
                        int m, int n, const int* mapCor, const int* photo)
{
	(void)ea;
	if (m <= 0 || n < 0 || !dpa || (n && (!W || !IV || !eb || !dpb || !mapCor || !photo))) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return solve_features(ctx, W, IV, eb, dpa, dpb, m, n, mapCor, photo); });
}

int lsfm_schur_pattern(lsfm_context* ctx, const int* Ui, const int* Uj, const int* photo, const int* feature, int m, int n, int nU, int nW, int* rowptr,
                       int* colidx, int cap, int* nnzb)
{
	if (m <= 0 || n < 0 || nU < 0 || nW < 0 || !rowptr || !colidx || !nnzb || (nU && (!Ui || !Uj)) || (nW && (!photo || !feature))) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		HostSystem h;
		h.m = m; h.n = n; h.nU = nU; h.nW = nW;
		h.Ui = Ui; h.Uj = Uj; h.photo = photo; h.feature = feature;
		SolveIO io;
		system_upload(ctx, h, 0, system_fptr(h, true), nullptr, io); // (a feature without a W block adds nothing to the pattern)
		int cnt = 0;
		const int* d_rowptr = nullptr;
		const int* d_colidx = nullptr;
		schur_pattern_only(ctx, io, &cnt, &d_rowptr, &d_colidx);
		*nnzb = cnt;
		if (cnt > cap) LSFM_FAIL(LSFM_ERR_ARG, "colidx too small for the pattern (" + std::to_string(cnt) + " blocks)");
		d2h(ctx, rowptr, d_rowptr, (size_t)(m + 1) * sizeof(int));
		d2h(ctx, colidx, d_colidx, (size_t)cnt * sizeof(int));
		return LSFM_OK;
	});
}

int lsfm_spmv_bench(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const double* x, double* y,
                    int reps, double* avg_ms, double* algorithmic_bytes)
{
	if (!rowptr || !colidx || !val || !x || !y || m <= 0) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		ctx->ensure_arenas(((size_t)rowptr[m] * 480 + (size_t)m * 1000) * 2 + ((size_t)64 << 20));
		ctx->scratch.reset();
		return spmv_external(ctx, m, rowptr, colidx, val, x, y, reps, avg_ms, algorithmic_bytes);
	});
}

// the matrix of the test entries on a caller's system: upper block CSR, every block row starting with its diagonal block, the
// columns of a row ascending
static bool block_csr_ok(int m, const int* rowptr, const int* colidx, const double* val)
{
	if (m <= 0 || !rowptr || !colidx || !val || rowptr[0] != 0) return false;
	for (int p = 0; p < m; p++)
	{
		if (rowptr[p + 1] <= rowptr[p] || colidx[rowptr[p]] != p) return false;
		for (int k = rowptr[p] + 1; k < rowptr[p + 1]; k++)
			if (colidx[k] <= colidx[k - 1] || colidx[k] >= m) return false;
	}
	return true;
}

int lsfm_selftest_chol(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                       const int* pose_seg, int nseg, const double* r, int nrhs, int mode, double* z, double* dot, int* perm, int* colptr, int* rowidx,
                       double* L, double* Dinv, double* dscale, int cap_blocks, int* info)
{
	if (!block_csr_ok(m, rowptr, colidx, val) || !pose_seg || nseg <= 0 || !r || nrhs <= 0 || mode < 0 || mode > 3 || !z || !dot || !info || cap_blocks < 0)
		return LSFM_ERR_ARG;
	for (int p = 0; p < m; p++)
		if (pose_seg[p] < 0 || pose_seg[p] >= nseg) return LSFM_ERR_ARG;
	for (int i = 0; i < LSFM_SELFTEST_CHOL_INFO; i++) info[i] = 0;
	return guarded(ctx, [&]() {
		return chol_selftest(ctx, m, rowptr, colidx, val, origin, fixed, pose_seg, nseg, r, nrhs, mode, z, dot, perm, colptr, rowidx, L, Dinv, dscale, cap_blocks, info);
	});
}

int lsfm_selftest_cc_sweeps(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin,
                            const unsigned char* fixed, const double* B, int R, const double* X, double* x, double* fwd, int* perm, double* dscale,
                            double* y, int* info)
{
	if (!block_csr_ok(m, rowptr, colidx, val) || !B || R < 1 || R > 192 /* 6 CC_KC: one chunk of columns */ || (X != nullptr) != (y != nullptr) || !info) return LSFM_ERR_ARG;
	for (int i = 0; i < LSFM_SELFTEST_CC_SWEEPS_INFO; i++) info[i] = 0;
	return guarded(ctx, [&]() { return cc_sweeps_selftest(ctx, m, rowptr, colidx, val, origin, fixed, B, R, X, x, fwd, perm, dscale, y, info); });
}

int lsfm_selftest_transform(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, const int* tref, const int* tscap, const int* tfix,
                            int alias_passthrough, lsfm_map* out)
{
	if (!maps || N <= 0 || !tref || !out || (mono && (!tscap || !tfix))) return LSFM_ERR_ARG;
	for (int b = 0; b < N; b++) memset(&out[b], 0, sizeof out[b]);
	int rc = guarded(ctx, [&]() {
		ctx->ensure_arenas(estimate_arena(maps, N, 1));
		ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
		DevBatch X, Y;
		batch_upload(ctx, ctx->arena[0], maps, N, mono != 0, X);
		std::vector<int> r(tref, tref + N), s(N, 0), f(N, 0);
		if (mono) { s.assign(tscap, tscap + N); f.assign(tfix, tfix + N); }
		transform_batch(ctx, ctx->arena[1], X, r, s, f, mono != 0, Y, alias_passthrough != 0);
		// the download reads W of the result; the blocks a passed-through map left behind come from the input, at the offset the
		// alias records (what a join's kernels do with W_alias / d_alias)
		std::vector<int> delta(N, INT_MIN);
		if (Y.W_alias) d2h(ctx, delta.data(), Y.d_alias, (size_t)N * sizeof(int));
		for (int b = 0; b < N; b++)
		{
			batch_download_map(ctx, Y, b, mono != 0, &out[b]);
			if (delta[b] == INT_MIN || !out[b].nW) continue;
			d2h(ctx, out[b].W, Y.W_alias + ((ptrdiff_t)Y.w_off[b] + delta[b]) * 18, (size_t)out[b].nW * 18 * sizeof(double));
		}
		return LSFM_OK;
	});
	if (rc < 0) for (int b = 0; b < N; b++) lsfm_map_release(&out[b]);
	return rc;
}

int lsfm_selftest_small(lsfm_context* ctx, int G, const int* pose_off, const int* feat_off, const int* u_off, const unsigned char* active,
                        const double* U, const int* Ui, const int* Uj, const double* W, const int* photo, const int* feature, int nW, const double* V,
                        const double* ea, const double* eb, const double* x0, const unsigned char* fixed, int strips, double* x_pose, double* x_feat,
                        int* status, double* max_rel)
{
	if (G <= 0 || !pose_off || !feat_off || !u_off || !ea || !x_pose || !status || !max_rel || strips < 0 || nW < 0) return LSFM_ERR_ARG;
	const int M = pose_off[G], NF = feat_off[G], NU = u_off[G];
	if (M <= 0 || NF < 0 || NU < 0 || (NU && (!U || !Ui || !Uj)) || (nW && (!W || !photo || !feature)) || (NF && (!V || !eb || !x_feat))) return LSFM_ERR_ARG;
	status[0] = status[1] = 0; *max_rel = 0.0;
	return guarded(ctx, [&]() {
		HostSystem h;
		h.m = M; h.n = NF; h.nU = NU; h.nW = nW;
		h.Ui = Ui; h.Uj = Uj; h.photo = photo; h.feature = feature;
		h.U = U; h.W = W; h.V = V; h.ea = ea; h.eb = eb; h.x0 = x0;
		return small_selftest(ctx, G, pose_off, feat_off, u_off, active, h, fixed, strips, x_pose, x_feat, status, max_rel);
	});
}

int lsfm_wstream_bench(lsfm_context* ctx, long long nblocks, int mode, int reps, double* avg_ms)
{
	if (nblocks <= 0 || mode < 0 || mode > 2 || reps <= 0 || !avg_ms) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() {
		ctx->ensure_arenas((size_t)nblocks * 144 * 2 + ((size_t)64 << 20));
		ctx->scratch.reset();
		return wstream_bench(ctx, nblocks, mode, reps, avg_ms);
	});
}
int lsfm_selftest_prims(lsfm_context* ctx, int cases, unsigned seed)
{
	if (cases <= 0) return LSFM_ERR_ARG;
	return guarded(ctx, [&]() { return prims_selftest(ctx, cases, seed); });
}

} // extern "C"
