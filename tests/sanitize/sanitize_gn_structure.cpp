// Stand-alone host program for AddressSanitizer + UndefinedBehaviorSanitizer over linearsfm_amd/csrc/lsfm_gn_structure.cpp (built with
// lsfm_system.cpp by tests/test_gn_structure_cpu.py): tiny label sets written out here -- a Stereo set with a map in the global frame, a
// repeated (pose, feature) pair and a map without features; a Mono set; a set that is refused -- through gn_structure and through the C
// entry lsfm_gn_structure with every output array at its exact size.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lsfm.h"
#include "../../linearsfm_amd/csrc/lsfm_gn_structure.hpp"

namespace {
struct Labels {
	std::vector<int> stno, Ui, Uj, photo, feature;
	std::vector<double> stVal;
	lsfm_map map;
};
// poses by id, features by id, U pairs and W (pose, feature) pairs by local index
void make(Labels& L, int Ref, int ScaP, int Fix, const std::vector<int>& poses, const std::vector<int>& feats, const std::vector<std::pair<int, int>>& U,
          const std::vector<std::pair<int, int>>& W)
{
	L.stno.clear();
	for (int p : poses) for (int i = 0; i < 6; i++) L.stno.push_back(-p);
	for (int f : feats) for (int i = 0; i < 3; i++) L.stno.push_back(f);
	L.stVal.assign(L.stno.size(), 0.0);
	L.Ui.clear(); L.Uj.clear(); L.photo.clear(); L.feature.clear();
	for (auto& u : U) { L.Ui.push_back(u.first); L.Uj.push_back(u.second); }
	for (auto& w : W) { L.photo.push_back(w.first); L.feature.push_back(w.second); }
	memset(&L.map, 0, sizeof L.map);
	L.map.Ref = L.map.FRef = Ref; L.map.ScaP = L.map.FScaP = ScaP; L.map.Fix = L.map.FFix = Fix; L.map.Sign = 1;
	L.map.m = (int)poses.size(); L.map.n = (int)feats.size(); L.map.nU = (int)U.size(); L.map.nW = (int)W.size();
	L.map.stno = L.stno.data(); L.map.stVal = L.stVal.data();
	L.map.Ui = L.Ui.data(); L.map.Uj = L.Uj.data(); L.map.photo = L.photo.data(); L.map.feature = L.feature.data();
}
int fail(const char* what) { fprintf(stderr, "sanitize_gn_structure: %s\n", what); return 1; }

// the C entry, sizes first, then every array at its exact size
int through_c(const std::vector<lsfm_map>& maps, int type, const lsfm_map& x, int slots, int coalesce, int* info)
{
	char why[256];
	const int N = (int)maps.size();
	int rc = lsfm_gn_structure(maps.data(), N, type, &x, slots, coalesce, info, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr,
	                           nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, why, (int)sizeof why);
	if (rc != LSFM_OK) { fprintf(stderr, "%s\n", why); return rc; }
	std::vector<int> hubs(3 * N), wdst(info[3]), fptrJ(info[1] + 1), photoJ(info[5]), UiJ(info[4]), UjJ(info[4]), photo(info[7]), feature(info[7]),
	    FBlock(info[1]), Ui(info[6]), Uj(info[6]), sm(info[8]), sa(info[8]), sb(info[8]), sc(info[8]);
	rc = lsfm_gn_structure(maps.data(), N, type, &x, slots, coalesce, info, hubs.data(), wdst.data(), fptrJ.data(), photoJ.data(), (int)photoJ.size(), UiJ.data(),
	                       UjJ.data(), (int)UiJ.size(), photo.data(), feature.data(), coalesce ? FBlock.data() : nullptr, (int)photo.size(), Ui.data(), Uj.data(),
	                       (int)Ui.size(), sm.data(), sa.data(), sb.data(), sc.data(), (int)sm.size(), why, (int)sizeof why);
	if (rc != LSFM_OK) { fprintf(stderr, "%s\n", why); return rc; }
	for (size_t q = 0; q < UiJ.size(); q++) if (UiJ[q] > UjJ[q]) return -100;
	int total = 0;
	for (int c : sc) total += c;
	return total == info[9] ? LSFM_OK : -101;
}
} // namespace

int main()
{
	using namespace lsfm;
	// ---- Stereo: global poses 1, 2, 3 (Ref 0 is no variable), features 1, 2 ----
	Labels x, a, b, c;
	make(x, 0, 0, 0, { 1, 2, 3 }, { 1, 2 }, {}, {});
	make(a, 0, 0, 0, { 1, 2 }, { 1, 2 }, { { 0, 0 }, { 0, 1 }, { 1, 1 } }, { { 1, 0 }, { 0, 0 }, { 1, 0 }, { 1, 1 } }); // the global frame; (pose 1, feature 0) twice
	make(b, 2, 0, 0, { 3 }, { 2 }, { { 0, 0 } }, { { 0, 0 } });
	make(c, 1, 0, 0, { 2, 3 }, {}, { { 0, 0 }, { 0, 1 }, { 1, 1 } }, {}); // no feature
	std::vector<lsfm_map> maps = { a.map, b.map, c.map };
	for (int slots = 0; slots < 2; slots++)
		for (int co = 0; co < 2; co++)
		{
			GnStructure st;
			std::string why;
			if (gn_structure(maps.data(), 3, false, &x.map, slots != 0, co != 0, st, why) != LSFM_OK) return fail(why.c_str());
			if (st.map[0].nh != 0 || st.map[1].nh != 1 || st.map[2].nh != 1 || st.P != 5 || st.FI != 3) return fail("Stereo: hubs or counts");
			// map a: slots (0,0) (0,1) (1,1) with 1, 1, 2 contributors (the repeated pair once); map b: (0,0); map c: none
			const int NS = (int)st.sl.a.size();
			if (NS != (slots ? 4 : 0) || (slots && (st.sl.cf.size() != 5 || st.sl.before[3] != 4))) return fail("Stereo: slots");
			if (st.NUJ != 3 + (1 + 1 + 1) + (2 + 1 + 3) + NS || st.NWJ != 4 + (1 + 1)) return fail("Stereo: joint counts");
			if (co && (st.co.nWo != 4 || st.co.FBlock.size() != 2)) return fail("Stereo: coalesced W");
			int info[10];
			if (through_c(maps, 0, x.map, slots, co, info) != LSFM_OK || info[8] != NS) return fail("Stereo: C entry");
		}
	// ---- Mono: global poses 1 (Ref), 2 (ScaP), 3, feature 1 ----
	Labels xm, am;
	make(xm, 1, 2, 0, { 1, 2, 3 }, { 1 }, {}, {});
	make(am, 1, 2, 1, { 2, 3 }, { 1 }, { { 0, 0 }, { 0, 1 }, { 1, 1 } }, { { 0, 0 }, { 1, 0 } });
	std::vector<lsfm_map> mm = { am.map };
	{
		GnStructure st;
		std::string why;
		if (gn_structure(mm.data(), 1, true, &xm.map, true, true, st, why) != LSFM_OK) return fail(why.c_str());
		if (st.map[0].nh != 2 || st.fixed.size() != 21 || st.NUJ != 2 * 2 + 3 + 3 + 3 || st.NWJ != 4) return fail("Mono: counts");
		int info[10];
		if (through_c(mm, 1, xm.map, 1, 1, info) != LSFM_OK) return fail("Mono: C entry");
	}
	// ---- refusals: a feature that is not in the state; a W run out of order ----
	{
		Labels bad;
		make(bad, 2, 0, 0, { 3 }, { 7 }, { { 0, 0 } }, { { 0, 0 } });
		std::vector<lsfm_map> r = { a.map, bad.map, c.map };
		GnStructure st;
		std::string why;
		if (gn_structure(r.data(), 3, false, &x.map, true, true, st, why) != LSFM_ERR_ARG || why != "gn polish: a feature of local map 2 is not in the global state")
			return fail("refusal: feature");
		make(bad, 2, 0, 0, { 3 }, { 1, 2 }, { { 0, 0 } }, { { 0, 1 }, { 0, 0 } });
		r[1] = bad.map;
		int info[10]; // (malformed index arrays are the entry's to refuse: gn_structure takes checked maps)
		if (through_c(r, 0, x.map, 1, 1, info) != LSFM_ERR_ARG) return fail("refusal: C entry");
	}
	printf("sanitize_gn_structure: ok\n");
	return 0;
}
