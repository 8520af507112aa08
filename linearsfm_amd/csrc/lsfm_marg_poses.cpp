// Marginalising poses out of a map: flags, components, boundaries and the pattern of U' from labels alone (lsfm_marg_poses.hpp).
// Plain C++: no device, no HIP header.
#include "lsfm_marg_poses.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "../../include/lsfm.h"
#include "lsfm_system.hpp"

namespace lsfm {

namespace {
inline unsigned long long pair_key(int i, int j) { return ((unsigned long long)(unsigned)i << 32) | (unsigned)j; }
} // namespace

int pose_marg_flags(const lsfm_map* map, bool mono, const unsigned char* keep_pose, const unsigned char* drop_feat, std::vector<unsigned char>& drop,
                    std::string& why)
{
	const int m = map->m, n = map->n;
	if (!keep_pose) { why = "keep_pose is NULL"; return LSFM_ERR_ARG; }
	if (m <= 0 || n < 0 || map->nW < 0 || !map->stno || (map->nW && (!map->photo || !map->feature))) { why = "the map has no poses, no labels or no index arrays"; return LSFM_ERR_ARG; }
	// ---- gauge: what the solvers hold fixed cannot leave ----
	int nkept = 0;
	for (int p = 0; p < m; p++) nkept += keep_pose[p] ? 1 : 0;
	if (!nkept) { why = "no pose is kept: a map has at least one"; return LSFM_ERR_ARG; }
	for (int p = 0; p < m; p++)
	{
		if (keep_pose[p]) continue;
		const int id = -map->stno[6 * p];
		if (id == map->Ref) { why = "the Ref pose " + std::to_string(id) + " must be kept"; return LSFM_ERR_ARG; }
		if (mono && id == map->ScaP) { why = "the ScaP pose " + std::to_string(id) + " of a Mono map must be kept"; return LSFM_ERR_ARG; }
	}
	// ---- features: one that a dropped pose sees goes with it ----
	std::vector<unsigned char> seen((size_t)n, 0);
	for (int w = 0; w < map->nW; w++)
	{
		const int f = map->feature[w], p = map->photo[w];
		if (f < 0 || f >= n || p < 0 || p >= m) { why = "a W block's pose or feature index is out of range"; return LSFM_ERR_ARG; }
		if (!keep_pose[p]) seen[f] = 1;
	}
	drop.assign((size_t)n, 0);
	for (int f = 0; f < n; f++)
	{
		if (!drop_feat) { drop[f] = seen[f]; continue; }
		if (seen[f] && !drop_feat[f])
		{
			why = "feature " + std::to_string(map->stno[6 * (size_t)m + 3 * (size_t)f]) + " (index " + std::to_string(f) + ") is kept but seen by a dropped pose: the result would not be a map";
			return LSFM_ERR_ARG;
		}
		drop[f] = drop_feat[f] ? 1 : 0;
	}
	return LSFM_OK;
}

std::vector<unsigned long long> marg_pattern_host(const lsfm_map* map, const std::vector<int>& fptr, const unsigned char* drop)
{
	std::vector<unsigned long long> keys;
	keys.reserve((size_t)map->m + map->nU);
	for (int p = 0; p < map->m; p++) keys.push_back(pair_key(p, p));
	for (int e = 0; e < map->nU; e++) keys.push_back(pair_key(map->Ui[e], map->Uj[e]));
	std::vector<int> ps;
	for (int f = 0; f < map->n; f++)
	{
		if (!drop[f]) continue;
		ps.assign(map->photo + fptr[f], map->photo + fptr[f + 1]);
		std::sort(ps.begin(), ps.end());
		ps.erase(std::unique(ps.begin(), ps.end()), ps.end());
		for (size_t a = 0; a < ps.size(); a++)
			for (size_t b = a + 1; b < ps.size(); b++) keys.push_back(pair_key(ps[a], ps[b]));
	}
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	return keys;
}

void pose_marg_structure(int m, int nU, const int* Ui, const int* Uj, const unsigned char* keep_pose, PoseMargStructure& st)
{
	st = PoseMargStructure();
	st.m = m;
	st.local.assign(m, 0); st.comp.assign(m, -1); st.bdpos.assign(m, -1);
	for (int p = 0; p < m; p++)
	{
		std::vector<int>& l = keep_pose[p] ? st.klist : st.dlist;
		st.local[p] = (int)l.size();
		l.push_back(p);
	}
	// ---- components of the graph on D (union-find, the smaller root wins: a root is its component's smallest pose) ----
	std::vector<int> par(m);
	std::iota(par.begin(), par.end(), 0);
	auto find = [&](int x) {
		while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; }
		return x;
	};
	for (int e = 0; e < nU; e++)
	{
		if (keep_pose[Ui[e]] || keep_pose[Uj[e]]) continue;
		const int a = find(Ui[e]), b = find(Uj[e]);
		if (a != b) par[std::max(a, b)] = std::min(a, b);
	}
	for (int p : st.dlist)
	{
		const int r = find(p);
		if (r == p) st.comp[p] = st.ncomp++;
		else st.comp[p] = st.comp[r]; // (r < p: numbered already)
	}
	// ---- boundaries ----
	std::vector<unsigned long long> nb; // (component, kept pose)
	for (int e = 0; e < nU; e++)
	{
		const int i = Ui[e], j = Uj[e];
		if (!keep_pose[i] && keep_pose[j]) nb.push_back(pair_key(st.comp[i], j));
		else if (keep_pose[i] && !keep_pose[j]) nb.push_back(pair_key(st.comp[j], i));
	}
	std::sort(nb.begin(), nb.end());
	nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
	st.nptr.assign((size_t)st.ncomp + 1, 0);
	st.nidx.resize(nb.size());
	for (size_t k = 0; k < nb.size(); k++)
	{
		st.nptr[(size_t)(nb[k] >> 32) + 1]++;
		st.nidx[k] = (int)(nb[k] & 0xffffffffull);
	}
	for (int c = 0; c < st.ncomp; c++) st.nptr[c + 1] += st.nptr[c];
	st.bd = st.nidx;
	std::sort(st.bd.begin(), st.bd.end());
	st.bd.erase(std::unique(st.bd.begin(), st.bd.end()), st.bd.end());
	for (size_t k = 0; k < st.bd.size(); k++) st.bdpos[st.bd[k]] = (int)k;
	// ---- the pattern of U', in the output's numbering (the renumbering ascends with the pose: the orders agree) ----
	std::vector<unsigned long long> fill;
	for (int c = 0; c < st.ncomp; c++)
		for (int a = st.nptr[c]; a < st.nptr[c + 1]; a++)
			for (int b = a; b < st.nptr[c + 1]; b++) fill.push_back(pair_key(st.local[st.nidx[a]], st.local[st.nidx[b]]));
	std::sort(fill.begin(), fill.end());
	fill.erase(std::unique(fill.begin(), fill.end()), fill.end());
	std::vector<std::pair<unsigned long long, int>> have; // the blocks of U1_KK
	for (int e = 0; e < nU; e++)
		if (keep_pose[Ui[e]] && keep_pose[Uj[e]]) have.emplace_back(pair_key(st.local[Ui[e]], st.local[Uj[e]]), e);
	std::sort(have.begin(), have.end());
	std::vector<unsigned long long> keys = fill;
	for (const auto& h : have) keys.push_back(h.first);
	for (size_t k = 0; k < st.klist.size(); k++) keys.push_back(pair_key((int)k, (int)k));
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	const size_t no = keys.size();
	st.oUi.resize(no); st.oUj.resize(no); st.osrc.assign(no, -1); st.ofill.assign(no, 0);
	size_t hp = 0, fp = 0;
	for (size_t k = 0; k < no; k++)
	{
		st.oUi[k] = (int)(keys[k] >> 32); st.oUj[k] = (int)(keys[k] & 0xffffffffull);
		while (hp < have.size() && have[hp].first < keys[k]) hp++;
		if (hp < have.size() && have[hp].first == keys[k]) st.osrc[k] = have[hp].second;
		while (fp < fill.size() && fill[fp] < keys[k]) fp++;
		if (fp < fill.size() && fill[fp] == keys[k]) st.ofill[k] = 1;
	}
}

} // namespace lsfm

extern "C" int lsfm_marg_pose_structure(const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat, unsigned char* drop,
                                        int* comp, int* nptr, int* nidx, int cap_n, int* bd, int* Ui, int* Uj, int cap_u, int* info, char* why, int why_cap)
{
	using namespace lsfm;
	auto fail = [&](const std::string& msg) {
		if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "%s", msg.c_str());
		return (int)LSFM_ERR_ARG;
	};
	if (why && why_cap > 0) why[0] = 0;
	if (!map || (mono != 0 && mono != 1)) return fail("map is NULL or mono is not 0 / 1");
	std::vector<unsigned char> dr;
	std::string msg;
	if (pose_marg_flags(map, mono == 1, keep_pose, drop_feat, dr, msg) != LSFM_OK) return fail(msg);
	std::vector<int> fptr;
	const char* bad = nullptr;
	if (system_check(host_system_of(*map, false), false, fptr, &bad) != LSFM_OK) return fail(bad ? bad : "malformed map");
	const std::vector<unsigned long long> keys = marg_pattern_host(map, fptr, dr.data());
	std::vector<int> ui(keys.size()), uj(keys.size());
	for (size_t k = 0; k < keys.size(); k++) { ui[k] = (int)(keys[k] >> 32); uj[k] = (int)(keys[k] & 0xffffffffull); }
	PoseMargStructure st;
	pose_marg_structure(map->m, (int)keys.size(), ui.data(), uj.data(), keep_pose, st);
	if (info)
	{
		int nd = 0, nf = 0;
		for (unsigned char d : dr) nd += d;
		for (char f : st.ofill) nf += f;
		info[0] = (int)st.dlist.size(); info[1] = (int)st.bd.size(); info[2] = st.ncomp; info[3] = (int)st.oUi.size();
		info[4] = (int)st.nidx.size(); info[5] = nd; info[6] = (int)keys.size(); info[7] = nf;
	}
	if (drop && map->n) memcpy(drop, dr.data(), (size_t)map->n);
	if (comp) memcpy(comp, st.comp.data(), (size_t)map->m * sizeof(int));
	if (nptr) memcpy(nptr, st.nptr.data(), st.nptr.size() * sizeof(int));
	if (bd && !st.bd.empty()) memcpy(bd, st.bd.data(), st.bd.size() * sizeof(int));
	if (nidx)
	{
		if (cap_n < (int)st.nidx.size()) return fail("cap_n is too small: " + std::to_string(st.nidx.size()) + " entries needed");
		if (!st.nidx.empty()) memcpy(nidx, st.nidx.data(), st.nidx.size() * sizeof(int));
	}
	if (Ui || Uj)
	{
		if (cap_u < (int)st.oUi.size()) return fail("cap_u is too small: " + std::to_string(st.oUi.size()) + " blocks needed");
		if (Ui) memcpy(Ui, st.oUi.data(), st.oUi.size() * sizeof(int));
		if (Uj) memcpy(Uj, st.oUj.data(), st.oUj.size() * sizeof(int));
	}
	return LSFM_OK;
}
