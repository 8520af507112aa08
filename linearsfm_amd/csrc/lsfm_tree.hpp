// The tree scheduler that replaces lmj_PF3D_Divide_Conquer{Stereo,Mono} (Imp.cpp:1926-2063 / 6511-6630): every level of the reference's
// binary join tree runs as ONE batch (lsfm_tree.hip).  The C ABI (lsfm_capi.hip) holds the tree's handle and calls tree_run.
#pragma once
#include <chrono>

#include "lsfm_internal.hpp"

struct lsfm_tree {
	bool mono = false;
	int N = 0;
	lsfm::Arena input_arena; // pristine copy of the N local maps, resident in HBM; lsfm_tree_run starts from a device copy of it
	lsfm::DevBatch input;
	lsfm::DevBatch level;    // current level (lives in ctx->arena[slot]; slot -1: the resident inputs)
	int slot = 0;
	bool done = false;
	bool final_reanchor = true;
	int stop_level = 0; // > 0: a run ends after this many tree levels (lsfm_tree_set_stop_level)
	unsigned long long generation = 0; // ctx->generation when the run ended: the result lives in the context's arenas
	// what the first run leaves for the next ones (structure only: the resident inputs never change): one plan per tree
	// level + one for the final re-anchoring transform
	std::vector<lsfm::LevelPlan> plans;
	bool use_plans = true;
	double upload_ms = 0; // wall time of lsfm_tree_upload (reported in lsfm_stats)
	// per level: the refinement steps the level's systems needed in an earlier run (0: not known).  Not structure -- a guess about
	// values that lets a run enqueue the steps of a level without stopping to ask; checked at the end of every run that uses it
	std::vector<int> step_hint;
	unsigned long long digest = 0; // of the resident inputs' labels and index arrays (trees built from packed maps: reload compares)
	// feature-sharded tree (lsfm_tree_set_comm): this process holds one slice of every map; comm.fn == null: off
	lsfm::Comm comm;
	// sizes of the slice packs of the final map (lsfm_tree_export_slice_*): structure, learnt at the first export
	int slice_n = 0;
	std::vector<int> slice_nf, slice_nw;
};

namespace lsfm {

inline double now_ms()
{
	using namespace std::chrono;
	return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

inline int tree_levels(int N)
{
	int L = 0;
	while (N > 1) { N = (N + 1) / 2; L++; }
	return L;
}
// what ensure_arenas is asked for on behalf of a tree: totals over its local maps
inline size_t estimate_arena(size_t nw, size_t nf, size_t nu, size_t m, int levels)
{
	const size_t L = levels + 1;
	return (nw + 2 * L * nf) * 160 * 3 + (nu + 3 * L * m) * 320 * 3 + nf * 400 + ((size_t)256 << 20);
}
inline size_t estimate_arena(const lsfm_map* maps, int N, int levels)
{
	size_t nw = 0, nf = 0, nu = 0, m = 0;
	for (int k = 0; k < N; k++) { nw += maps[k].nW; nf += maps[k].n; nu += maps[k].nU; m += maps[k].m; }
	return estimate_arena(nw, nf, nu, m, levels);
}
// lsfm_tree_run: joins the resident tree, repeating the run where its record asks for it; LSFM_OK or LSFM_NOT_CONVERGED
int tree_run(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* stats);

} // namespace lsfm
