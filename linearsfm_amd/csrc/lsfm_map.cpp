// The allocator of every map the library hands out and its counterpart (lsfm_map.hpp).  Plain C++: no device, no HIP header.
#include "lsfm_map.hpp"

#include <cstdlib>

namespace lsfm {

namespace {
template <class T> T* host_alloc(size_t n) { return static_cast<T*>(malloc((n ? n : 1) * sizeof(T))); }
} // namespace

int map_alloc(lsfm_map& g, const lsfm_map* like, int m, int n, int nU, int nW, bool pose_origin)
{
	memset(&g, 0, sizeof g);
	if (like)
	{
		g.Ref = like->Ref; g.FRef = like->FRef;
		g.ScaP = like->ScaP; g.Fix = like->Fix; g.Sign = like->Sign; g.FScaP = like->FScaP; g.FFix = like->FFix;
	}
	g.m = m; g.n = n; g.nU = nU; g.nW = nW;
	const size_t r = (size_t)6 * m + (size_t)3 * n;
	g.stno = host_alloc<int>(r); g.stVal = host_alloc<double>(r);
	g.U = host_alloc<double>((size_t)nU * 36); g.Ui = host_alloc<int>(nU); g.Uj = host_alloc<int>(nU);
	g.W = host_alloc<double>((size_t)nW * 18); g.photo = host_alloc<int>(nW); g.feature = host_alloc<int>(nW);
	g.V = host_alloc<double>((size_t)n * 9); g.FBlock = host_alloc<int>(n);
	if (pose_origin) g.pose_origin = host_alloc<int>(m);
	if (g.stno && g.stVal && g.U && g.Ui && g.Uj && g.W && g.photo && g.feature && g.V && g.FBlock && (!pose_origin || g.pose_origin)) return LSFM_OK;
	lsfm_map_release(&g);
	return LSFM_ERR_OOM;
}

} // namespace lsfm

extern "C" void lsfm_map_release(lsfm_map* g)
{
	if (!g) return;
	free(g->stno); free(g->stVal); free(g->U); free(g->Ui); free(g->Uj); free(g->W); free(g->photo); free(g->feature);
	free(g->V); free(g->FBlock); free(g->pose_origin);
	memset(g, 0, sizeof *g);
}
