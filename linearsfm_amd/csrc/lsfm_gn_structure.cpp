// The structure of the Gauss-Newton polish's joint system from labels alone (lsfm_gn_structure.hpp).  Plain C++: no device, no HIP header.
#include "lsfm_gn_structure.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/lsfm.h"
#include "lsfm_system.hpp"

namespace lsfm {

namespace {
struct Lab { int id, idx; };
int lab_find(const std::vector<Lab>& t, int id)
{
	auto it = std::lower_bound(t.begin(), t.end(), id, [](const Lab& a, int v) { return a.id < v; });
	return (it != t.end() && it->id == id) ? it->idx : -1;
}

int gn_feature_slots(const lsfm_map* maps, int N, const GnStructure& st, GnSlots& sl, std::string& why)
{
	struct Tup { long long key; int f, ea, eb; };
	std::vector<Tup> tup;
	std::vector<std::pair<int, int>> run; // (local pose, W block)
	std::vector<int> ent, entpose;
	sl.before.assign(N + 1, 0); sl.sptr.clear(); sl.eptr.assign(1, 0);
	for (int k = 0; k < N; k++)
	{
		const lsfm_map& L = maps[k];
		tup.clear();
		int j = 0;
		for (int f = 0; f < L.n; f++)
		{
			run.clear();
			for (; j < L.nW && L.feature[j] == f; j++) run.push_back({ L.photo[j], st.w_off[k] + j });
			const auto by_pose = [](const std::pair<int, int>& p, const std::pair<int, int>& q) { return p.first < q.first; };
			if (!std::is_sorted(run.begin(), run.end(), by_pose)) std::stable_sort(run.begin(), run.end(), by_pose);
			ent.clear(); entpose.clear();
			for (size_t r = 0; r < run.size(); r++)
			{
				if (r == 0 || run[r].first != run[r - 1].first)
				{
					ent.push_back((int)sl.eptr.size() - 1); entpose.push_back(run[r].first);
					sl.eptr.push_back((int)sl.eidx.size());
				}
				sl.eidx.push_back(run[r].second);
				sl.eptr.back() = (int)sl.eidx.size();
			}
			for (size_t i = 0; i < ent.size(); i++)
				for (size_t q = i; q < ent.size(); q++) tup.push_back(Tup{ (long long)entpose[i] * L.m + entpose[q], st.feat_off[k] + f, ent[i], ent[q] });
		}
		const auto by_key = [](const Tup& p, const Tup& q) { return p.key < q.key; };
		if (!std::is_sorted(tup.begin(), tup.end(), by_key)) std::stable_sort(tup.begin(), tup.end(), by_key);
		if (sl.cf.size() + tup.size() > (size_t)INT32_MAX) { why = "gn polish: too many co-observations for the feature weights' correction of U"; return LSFM_ERR_ARG; }
		for (size_t i = 0; i < tup.size(); i++)
		{
			if (i == 0 || tup[i].key != tup[i - 1].key)
			{
				sl.a.push_back((int)(tup[i].key / L.m)); sl.b.push_back((int)(tup[i].key % L.m));
				sl.sptr.push_back((int)sl.cf.size());
			}
			sl.cf.push_back(tup[i].f); sl.ca.push_back(tup[i].ea); sl.cb.push_back(tup[i].eb);
		}
		sl.before[k + 1] = (int)sl.a.size();
	}
	sl.sptr.push_back((int)sl.cf.size());
	return LSFM_OK;
}

// the extended U list: every map's own blocks, then its slots
void gn_extended_u(const lsfm_map* maps, const GnStructure& st, GnSlots& sl)
{
	const int N = st.N, NS = (int)sl.a.size(), NUX = st.u_off[N] + NS;
	sl.Uix.assign(NUX, 0); sl.Ujx.assign(NUX, 0); sl.sdst.assign(NS, 0); sl.ushift.assign(N, 0);
	for (int k = 0; k < N; k++)
	{
		const GnMapShape& t = st.map[k];
		sl.ushift[k] = sl.before[k];
		for (int i = 0; i < maps[k].nU; i++) { sl.Uix[t.u0 + i] = t.p0 + maps[k].Ui[i]; sl.Ujx[t.u0 + i] = t.p0 + maps[k].Uj[i]; }
		for (int q = sl.before[k]; q < sl.before[k + 1]; q++)
		{
			const int d = t.u0 + maps[k].nU + (q - sl.before[k]);
			sl.sdst[q] = d; sl.Uix[d] = t.p0 + sl.a[q]; sl.Ujx[d] = t.p0 + sl.b[q];
		}
	}
}

void gn_coalesce(const GnStructure& st, GnCoalesced& co)
{
	const int NFG = st.NFG, NWJ = st.NWJ, NUJ = st.NUJ;
	const std::vector<int>&fptrJ = st.fptrJ, &photoJ = st.photoJ, &UiJ = st.UiJ, &UjJ = st.UjJ;
	// W: every feature's joint run sorted stably by pose, equal poses merged
	co.wsp.assign(1, 0); co.wsi.resize(NWJ); co.usp.assign(1, 0); co.usi.resize(NUJ);
	co.photo.clear(); co.feature.clear(); co.FBlock.assign(NFG, 0);
	for (int q = 0; q < NWJ; q++) co.wsi[q] = q;
	for (int g = 0; g < NFG; g++)
	{
		std::stable_sort(co.wsi.begin() + fptrJ[g], co.wsi.begin() + fptrJ[g + 1], [&](int a, int b) { return photoJ[a] < photoJ[b]; });
		co.FBlock[g] = (int)co.photo.size();
		for (int q = fptrJ[g]; q < fptrJ[g + 1]; q++)
		{
			if (q > fptrJ[g] && photoJ[co.wsi[q]] == photoJ[co.wsi[q - 1]]) continue;
			if (q > 0) co.wsp.push_back(q);
			co.photo.push_back(photoJ[co.wsi[q]]); co.feature.push_back(g);
		}
	}
	co.wsp.push_back(NWJ);
	if (NWJ == 0) co.wsp.assign(1, 0);
	// U: the joint keys sorted stably by (i, j), equal keys merged
	for (int q = 0; q < NUJ; q++) co.usi[q] = q;
	std::stable_sort(co.usi.begin(), co.usi.end(), [&](int a, int b) { return UiJ[a] != UiJ[b] ? UiJ[a] < UiJ[b] : UjJ[a] < UjJ[b]; });
	co.Ui.clear(); co.Uj.clear();
	for (int q = 0; q < NUJ; q++)
	{
		if (q > 0 && UiJ[co.usi[q]] == UiJ[co.usi[q - 1]] && UjJ[co.usi[q]] == UjJ[co.usi[q - 1]]) continue;
		if (q > 0) co.usp.push_back(q);
		co.Ui.push_back(UiJ[co.usi[q]]); co.Uj.push_back(UjJ[co.usi[q]]);
	}
	co.usp.push_back(NUJ);
	if (NUJ == 0) co.usp.assign(1, 0);
	co.nWo = (int)co.photo.size(); co.nUo = (int)co.Ui.size();
}
} // namespace

int gn_structure(const lsfm_map* maps, int N, bool mono, const lsfm_map* x, bool want_slots, bool want_coalesce, GnStructure& st, std::string& why)
{
	auto fail = [&](const std::string& msg) { why = msg; return (int)LSFM_ERR_ARG; };
	st = GnStructure();
	const int M = st.M = x->m, NFG = st.NFG = x->n;
	st.N = N; st.mono = mono;
	if (M <= 0 || NFG < 0 || !x->stno || !x->stVal) return fail("gn polish: the global state is empty");
	// ---- which global variable every local one is, where every local block lands ----
	std::vector<Lab> pt(M), ft(NFG);
	for (int i = 0; i < M; i++) { if (x->stno[6 * i] > 0) return fail("gn polish: state label of a pose must be <= 0"); pt[i] = Lab{ -x->stno[6 * i], i }; }
	for (int i = 0; i < NFG; i++) { if (x->stno[6 * M + 3 * i] <= 0) return fail("gn polish: state label of a feature must be > 0"); ft[i] = Lab{ x->stno[6 * M + 3 * i], i }; }
	auto by_id = [](const Lab& a, const Lab& b) { return a.id < b.id; };
	std::sort(pt.begin(), pt.end(), by_id); std::sort(ft.begin(), ft.end(), by_id);
	// the batch's offsets and the W run of every local feature instance (batch indices)
	st.pose_off.assign(N + 1, 0); st.feat_off.assign(N + 1, 0); st.u_off.assign(N + 1, 0); st.w_off.assign(N + 1, 0);
	for (int k = 0; k < N; k++)
	{
		st.pose_off[k + 1] = st.pose_off[k] + maps[k].m; st.feat_off[k + 1] = st.feat_off[k] + maps[k].n;
		st.u_off[k + 1] = st.u_off[k] + maps[k].nU; st.w_off[k + 1] = st.w_off[k] + maps[k].nW;
	}
	std::vector<int> fptr_loc(st.feat_off[N] + 1);
	for (int k = 0; k < N; k++)
	{
		int j = 0;
		for (int f = 0; f < maps[k].n; f++) { fptr_loc[st.feat_off[k] + f] = st.w_off[k] + j; while (j < maps[k].nW && maps[k].feature[j] == f) j++; }
	}
	fptr_loc[st.feat_off[N]] = st.w_off[N];
	const int P = st.P = st.pose_off[N], FI = st.FI = st.feat_off[N];
	GnSlots& sl = st.sl;
	st.has_slots = want_slots;
	if (want_slots) { if (gn_feature_slots(maps, N, st, sl, why) != LSFM_OK) return LSFM_ERR_ARG; }
	else sl.before.assign(N + 1, 0);
	st.map.resize(N); st.dof.resize(N);
	std::vector<int>&gp = st.gp, &gfi = st.gf, &wdst = st.wdst, &origin = st.origin, &fcnt = st.fsp, &pcnt = st.psp;
	gp.resize(P); gfi.resize(FI); wdst.resize(FI); origin.assign(M, INT32_MAX);
	fcnt.assign(NFG + 1, 0); pcnt.assign(M + 1, 0);
	int NUJ = 0;
	for (int k = 0; k < N; k++)
	{
		const lsfm_map& L = maps[k];
		GnMapShape& t = st.map[k];
		memset(&t, 0, sizeof t);
		t.p0 = st.pose_off[k]; t.m = L.m; t.f0 = st.feat_off[k]; t.n = L.n;
		t.u0 = st.u_off[k] + sl.before[k]; t.nu_own = L.nU; t.nu = L.nU + (sl.before[k + 1] - sl.before[k]);
		t.hub[0] = t.hub[1] = -1;
		if ((st.dof[k] = 6 * L.m + 3 * L.n) <= 0) return fail("gn polish: local map " + std::to_string(k + 1) + " is empty");
		if (!mono && L.Ref == x->Ref) t.nh = 0;
		else
		{
			t.nh = mono ? 2 : 1;
			if ((t.hub[0] = lab_find(pt, L.Ref)) < 0) return fail("gn polish: the reference pose of local map " + std::to_string(k + 1) + " is not in the global state");
			if (mono)
			{
				if ((t.hub[1] = lab_find(pt, L.ScaP)) < 0) return fail("gn polish: the scale pose of local map " + std::to_string(k + 1) + " is not in the global state");
				if (L.Fix < 0 || L.Fix > 2) return fail("gn polish: Fix must be 0, 1 or 2");
				t.fix = L.Fix;
			}
		}
		t.ubase = NUJ;
		NUJ += t.nh * L.m + t.nh * (t.nh + 1) / 2 + t.nu;
		for (int i = 0; i < L.m; i++)
		{
			const int g = lab_find(pt, -L.stno[6 * i]);
			if (g < 0) return fail("gn polish: a pose of local map " + std::to_string(k + 1) + " is not in the global state (Stereo: the global reference pose cannot be a variable of a map)");
			gp[t.p0 + i] = g; pcnt[g + 1]++;
			origin[g] = std::min(origin[g], k);
		}
		for (int sdx = 0; sdx < t.nh; sdx++) { pcnt[t.hub[sdx] + 1]++; origin[t.hub[sdx]] = std::min(origin[t.hub[sdx]], k); }
		for (int i = 0; i < L.n; i++)
		{
			const int g = lab_find(ft, L.stno[6 * L.m + 3 * i]);
			if (g < 0) return fail("gn polish: a feature of local map " + std::to_string(k + 1) + " is not in the global state");
			gfi[t.f0 + i] = g;
		}
	}
	st.NUJ = NUJ;
	// joint W: per global feature its instances in map order, an instance's hub block(s) ahead of its own run
	std::vector<int>& fptrJ = st.fptrJ;
	fptrJ.assign(NFG + 1, 0);
	for (int k = 0; k < N; k++)
		for (int f = st.feat_off[k]; f < st.feat_off[k + 1]; f++) { fptrJ[gfi[f] + 1] += st.map[k].nh + (fptr_loc[f + 1] - fptr_loc[f]); fcnt[gfi[f] + 1]++; }
	for (int g = 0; g < NFG; g++)
	{
		if (!fcnt[g + 1]) return fail("gn polish: a feature of the global state is in no local map");
		fptrJ[g + 1] += fptrJ[g]; fcnt[g + 1] += fcnt[g];
	}
	for (int g = 0; g < M; g++)
	{
		if (!pcnt[g + 1]) return fail("gn polish: a pose of the global state is in no local map");
		pcnt[g + 1] += pcnt[g];
	}
	const int NWJ = st.NWJ = fptrJ[NFG];
	std::vector<int>&photoJ = st.photoJ, &fsrc = st.fsi, &psrc = st.psi;
	photoJ.resize(NWJ); fsrc.resize(FI); psrc.resize(pcnt[M]);
	{
		std::vector<int> wcur(fptrJ.begin(), fptrJ.end() - 1), fcur(fcnt.begin(), fcnt.end() - 1), pcur(pcnt.begin(), pcnt.end() - 1);
		for (int k = 0; k < N; k++)
		{
			const GnMapShape& t = st.map[k];
			for (int f = t.f0; f < t.f0 + t.n; f++)
			{
				const int g = gfi[f], len = fptr_loc[f + 1] - fptr_loc[f];
				wdst[f] = wcur[g];
				for (int sdx = 0; sdx < t.nh; sdx++) photoJ[wcur[g]++] = t.hub[sdx];
				for (int j = 0; j < len; j++) photoJ[wcur[g]++] = gp[t.p0 + maps[k].photo[fptr_loc[f] - st.w_off[k] + j]];
				fsrc[fcur[g]++] = f;
			}
			for (int a = t.p0; a < t.p0 + t.m; a++) psrc[pcur[gp[a]]++] = a;
			for (int sdx = 0; sdx < t.nh; sdx++) psrc[pcur[t.hub[sdx]]++] = -1 - (2 * k + sdx);
		}
	}
	// joint U coordinates (row <= column)
	std::vector<int>&UiJ = st.UiJ, &UjJ = st.UjJ;
	UiJ.resize(NUJ); UjJ.resize(NUJ);
	for (int k = 0; k < N; k++)
	{
		const GnMapShape& t = st.map[k];
		int q = t.ubase;
		for (int sdx = 0; sdx < t.nh; sdx++)
			for (int a = 0; a < t.m; a++, q++) { const int ga = gp[t.p0 + a], h = t.hub[sdx]; UiJ[q] = std::min(ga, h); UjJ[q] = std::max(ga, h); }
		if (t.nh >= 1) { UiJ[q] = UjJ[q] = t.hub[0]; q++; }
		if (t.nh == 2) { UiJ[q] = std::min(t.hub[0], t.hub[1]); UjJ[q] = std::max(t.hub[0], t.hub[1]); q++; UiJ[q] = UjJ[q] = t.hub[1]; q++; }
		for (int i = 0; i < t.nu; i++, q++)
		{
			// (the map's own blocks, then its correction slots)
			const int own = t.nu_own, sq = sl.before[k] + i - own;
			const int ga = gp[t.p0 + (i < own ? maps[k].Ui[i] : sl.a[sq])], gb = gp[t.p0 + (i < own ? maps[k].Uj[i] : sl.b[sq])];
			UiJ[q] = std::min(ga, gb); UjJ[q] = std::max(ga, gb);
		}
	}
	if (x->pose_origin) for (int g = 0; g < M; g++) origin[g] = x->pose_origin[g];
	if (mono)
	{
		const int pr = lab_find(pt, x->Ref), ps = lab_find(pt, x->ScaP);
		if (pr < 0 || ps < 0 || x->Fix < 0 || x->Fix > 2) return fail("gn polish: the global state's reference / scale pose (Ref, ScaP, Fix) is not in it");
		st.fixed.assign((size_t)M * 6 + (size_t)NFG * 3, 0);
		for (int i = 0; i < 6; i++) st.fixed[(size_t)pr * 6 + i] = 1;
		st.fixed[(size_t)ps * 6 + x->Fix] = 1;
	}
	if (want_slots) gn_extended_u(maps, st, sl);
	st.has_coalesced = want_coalesce;
	if (want_coalesce) gn_coalesce(st, st.co);
	return LSFM_OK;
}

} // namespace lsfm

extern "C" int lsfm_gn_structure(const lsfm_map* maps, int N, int type, const lsfm_map* x, int want_slots, int want_coalesce, int* info, int* map_hubs,
                                 int* wdst, int* fptrJ, int* photoJ, int cap_wj, int* UiJ, int* UjJ, int cap_uj, int* photo, int* feature, int* FBlock,
                                 int cap_w, int* Ui, int* Uj, int cap_u, int* slot_map, int* slot_a, int* slot_b, int* slot_count, int cap_s, char* why,
                                 int why_cap)
{
	using namespace lsfm;
	auto fail = [&](const std::string& msg) {
		if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "%s", msg.c_str());
		return (int)LSFM_ERR_ARG;
	};
	if (why && why_cap > 0) why[0] = 0;
	if (!maps || N <= 0 || !x || (type != 0 && type != 1)) return fail("maps or x is NULL, N <= 0 or type is not 0 / 1");
	for (int k = 0; k < N; k++)
	{
		// (the device calls hand gn_structure maps that batch_upload has checked; here the same checks come from system_check)
		std::vector<int> fptr;
		const char* bad = nullptr;
		if (system_check(host_system_of(maps[k], false), false, fptr, &bad) != LSFM_OK) return fail(bad ? bad : "malformed map");
		if ((maps[k].m || maps[k].n) && !maps[k].stno) return fail("null index array");
	}
	GnStructure st;
	std::string msg;
	if (gn_structure(maps, N, type == 1, x, want_slots != 0, want_coalesce != 0, st, msg) != LSFM_OK) return fail(msg);
	const int NS = (int)st.sl.a.size();
	if (info)
	{
		const int v[10] = { st.M, st.NFG, st.P, st.FI, st.NUJ, st.NWJ, st.co.nUo, st.co.nWo, NS, (int)st.sl.cf.size() };
		memcpy(info, v, sizeof v);
	}
	auto put = [](int* dst, const std::vector<int>& src) { if (dst && !src.empty()) memcpy(dst, src.data(), src.size() * sizeof(int)); };
	if (map_hubs) for (int k = 0; k < N; k++) { map_hubs[3 * k] = st.map[k].nh; map_hubs[3 * k + 1] = st.map[k].hub[0]; map_hubs[3 * k + 2] = st.map[k].hub[1]; }
	put(wdst, st.wdst); put(fptrJ, st.fptrJ);
	if (photoJ) { if (cap_wj < st.NWJ) return fail("cap_wj is too small: " + std::to_string(st.NWJ) + " blocks needed"); put(photoJ, st.photoJ); }
	if (UiJ || UjJ) { if (cap_uj < st.NUJ) return fail("cap_uj is too small: " + std::to_string(st.NUJ) + " blocks needed"); put(UiJ, st.UiJ); put(UjJ, st.UjJ); }
	if (photo || feature) { if (cap_w < st.co.nWo) return fail("cap_w is too small: " + std::to_string(st.co.nWo) + " blocks needed"); put(photo, st.co.photo); put(feature, st.co.feature); }
	put(FBlock, st.co.FBlock);
	if (Ui || Uj) { if (cap_u < st.co.nUo) return fail("cap_u is too small: " + std::to_string(st.co.nUo) + " blocks needed"); put(Ui, st.co.Ui); put(Uj, st.co.Uj); }
	if (slot_map || slot_a || slot_b || slot_count)
	{
		if (cap_s < NS) return fail("cap_s is too small: " + std::to_string(NS) + " slots needed");
		for (int k = 0; k < N; k++)
			for (int q = st.sl.before[k]; q < st.sl.before[k + 1]; q++)
			{
				if (slot_map) slot_map[q] = k;
				if (slot_a) slot_a[q] = st.sl.a[q];
				if (slot_b) slot_b[q] = st.sl.b[q];
				if (slot_count) slot_count[q] = st.sl.sptr[q + 1] - st.sl.sptr[q];
			}
	}
	return LSFM_OK;
}
