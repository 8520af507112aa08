// A system from host arrays into arena 0 (lsfm_system.hpp): the one upload behind lsfm_solve_*, lsfm_map_covariance[_columns],
// lsfm_map_marginalise and lsfm_schur_pattern.
#include "lsfm_system.hpp"

#include <type_traits>

#include "lsfm_internal.hpp"

namespace lsfm {

std::vector<int> system_fptr(const HostSystem& h, bool empty_features_ok)
{
	std::vector<int> fptr;
	const char* why = "";
	if (system_check(h, empty_features_ok, fptr, &why) != LSFM_OK) LSFM_FAIL(LSFM_ERR_ARG, why);
	return fptr;
}

size_t system_arena_need(const HostSystem& h, unsigned pieces)
{
	const size_t m = h.m, n = h.n, nU = h.nU, nW = h.nW;
	if (!(pieces & SYS_VALUES)) return (nW * 64 + nU * 64 + m * 4096) * 2 + ((size_t)64 << 20);
	return (nW * 200 + nU * 400 + n * 300 + m * 4000) * 3 + ((size_t)128 << 20);
}

void system_upload(lsfm_context* ctx, const HostSystem& h, unsigned pieces, const std::vector<int>& fptr, const std::vector<unsigned char>* fixed,
                   SolveIO& io, const int** d_feature)
{
	const size_t m = h.m, n = h.n, nU = h.nU, nW = h.nW;
	ctx->ensure_arenas(system_arena_need(h, pieces));
	ctx->arena[0].reset(); ctx->scratch.reset();
	Arena& ar = ctx->arena[0];
	auto up = [&](auto* src, size_t count) {
		auto* d = ar.alloc<std::remove_cv_t<std::remove_pointer_t<decltype(src)>>>(count);
		h2d(ctx, d, src, count * sizeof *src);
		return d;
	};
	auto zeros = [&](size_t count) {
		double* d = ar.alloc<double>(count);
		dev_zero(ctx, d, count * sizeof(double));
		return d;
	};
	const bool values = pieces & SYS_VALUES;
	io = SolveIO();
	io.M = h.m; io.NF = h.n; io.NU = h.nU; io.NW = h.nW; io.nseg = 1;
	io.seg_rows.assign(1, h.m);
	if (values) io.U = up(h.U, nU * 36);
	io.Ui = up(h.Ui, nU); io.Uj = up(h.Uj, nU);
	if (values) io.W = up(h.W, nW * 18);
	io.photo = up(h.photo, nW);
	if (pieces & SYS_FEATURE) *d_feature = up(h.feature, nW);
	io.fptr = up(fptr.data(), n + 1);
	if (values) io.V = up(h.V, n * 9);
	if (pieces & SYS_RHS) { io.ea = up(h.ea, m * 6); io.eb = up(h.eb, n * 3); }
	if (pieces & SYS_RHS_0) { io.ea = zeros(m * 6); io.eb = zeros(n * 3); }
	if (pieces & SYS_X)
	{
		if (h.x0) io.x0 = up(h.x0, m * 6);
		io.x_pose = ar.alloc<double>(m * 6); io.x_feat = ar.alloc<double>(n * 3);
	}
	if (pieces & (SYS_RHS | SYS_RHS_0))
	{
		int* seg = ar.alloc<int>(m + n + 1);
		dev_zero(ctx, seg, (m + n + 1) * sizeof(int));
		io.d_pose_seg = seg; io.d_feat_seg = seg + m;
	}
	if (pieces & SYS_OFFSETS)
	{
		const int offs[6] = { 0, h.m, 0, h.n, 0, h.nU };
		const int* d_offs = up(offs, 6);
		io.d_pose_off = d_offs; io.d_feat_off = d_offs + 2; io.d_u_off = d_offs + 4;
	}
	if (h.pose_origin) io.d_pose_origin = up(h.pose_origin, m);
	if (fixed) io.d_fixed = up(fixed->data(), fixed->size());
}

} // namespace lsfm
