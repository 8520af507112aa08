// Stand-alone host program for AddressSanitizer + UndefinedBehaviorSanitizer (leak detection on) over linearsfm_amd/csrc/lsfm_map.cpp
// (built with lsfm_system.cpp by tests/test_map_cpu.py): the one allocator of the maps the library hands out at the smallest sizes and
// sizes with empty arrays, with and without pose_origin and a map to copy the scalars from; every array written over its whole length;
// the owner MapOut left without give() and after give(); lsfm_map_release twice on one struct; host_system_of on a map without features.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/lsfm.h"
#include "../../linearsfm_amd/csrc/lsfm_map.hpp"
#include "../../linearsfm_amd/csrc/lsfm_system.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sanitize_map: check failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
// every element of every array, so that an array shorter than its size says is a report
void fill(lsfm_map& g)
{
	const size_t r = (size_t)6 * g.m + (size_t)3 * g.n;
	for (size_t i = 0; i < r; i++) { g.stno[i] = (int)i; g.stVal[i] = 0.5 * (double)i; }
	for (size_t i = 0; i < (size_t)g.nU * 36; i++) g.U[i] = 1.0;
	for (int i = 0; i < g.nU; i++) { g.Ui[i] = 0; g.Uj[i] = g.m - 1; }
	for (size_t i = 0; i < (size_t)g.nW * 18; i++) g.W[i] = 2.0;
	for (int i = 0; i < g.nW; i++) { g.photo[i] = i % g.m; g.feature[i] = g.n ? (int)((long)i * g.n / g.nW) : 0; }
	for (size_t i = 0; i < (size_t)g.n * 9; i++) g.V[i] = 3.0;
	for (int i = 0; i < g.n; i++) g.FBlock[i] = i;
	if (g.pose_origin) for (int i = 0; i < g.m; i++) g.pose_origin[i] = i;
}
bool zeroed(const lsfm_map& g)
{
	lsfm_map z;
	memset(&z, 0, sizeof z);
	return memcmp(&g, &z, sizeof z) == 0;
}
} // namespace

int main()
{
	using namespace lsfm;
	lsfm_map like;
	memset(&like, 0, sizeof like);
	like.Ref = 3; like.FRef = 4; like.ScaP = 5; like.Fix = 2; like.Sign = -1; like.FScaP = 6; like.FFix = 1;
	like.m = 99; like.n = 98; like.nU = 97; like.nW = 96; // (the sizes are the call's, not the model's)
	const int sizes[3][4] = { { 1, 0, 0, 0 }, { 2, 1, 1, 1 }, { 3, 2, 4, 3 } };
	int made = 0;
	for (const auto& sz : sizes)
		for (int origin = 0; origin < 2; origin++)
			for (int with_like = 0; with_like < 2; with_like++)
			{
				lsfm_map g;
				memset(&g, 0xff, sizeof g); // (map_alloc starts from whatever is there)
				CHECK(map_alloc(g, with_like ? &like : nullptr, sz[0], sz[1], sz[2], sz[3], origin != 0) == LSFM_OK);
				CHECK(g.m == sz[0] && g.n == sz[1] && g.nU == sz[2] && g.nW == sz[3]);
				CHECK(g.stno && g.stVal && g.U && g.Ui && g.Uj && g.W && g.photo && g.feature && g.V && g.FBlock);
				CHECK((g.pose_origin != nullptr) == (origin != 0));
				if (with_like) CHECK(g.Ref == 3 && g.FRef == 4 && g.ScaP == 5 && g.Fix == 2 && g.Sign == -1 && g.FScaP == 6 && g.FFix == 1);
				else CHECK(g.Ref == 0 && g.FRef == 0 && g.ScaP == 0 && g.Fix == 0 && g.Sign == 0 && g.FScaP == 0 && g.FFix == 0);
				fill(g);
				const HostSystem h = host_system_of(g, true);
				CHECK(h.m == g.m && h.n == g.n && h.nU == g.nU && h.nW == g.nW && h.Ui == g.Ui && h.Uj == g.Uj && h.photo == g.photo && h.feature == g.feature);
				CHECK(h.U == g.U && h.W == g.W && h.V == g.V && !h.ea && !h.eb && !h.x0 && !h.pose_origin);
				std::vector<int> fptr;
				const char* why = nullptr;
				CHECK(system_check(h, false, fptr, &why) == LSFM_OK && (int)fptr.size() == g.n + 1 && fptr[g.n] == g.nW);
				lsfm_map_release(&g);
				CHECK(zeroed(g));
				lsfm_map_release(&g); // a second release of the same struct frees nothing
				CHECK(zeroed(g));
				made++;
			}
	// the owner: left without give(), the map goes with it (a leak would be reported at exit) ...
	{
		MapOut A;
		CHECK(zeroed(A.g));
		CHECK(map_alloc(A.g, &like, 3, 2, 4, 3, true) == LSFM_OK);
		fill(A.g);
	}
	{
		MapOut never; // ... and one that never held a map releases nothing
	}
	// ... after give() the map is the caller's, the owner is empty and its destructor leaves the caller's map alone
	lsfm_map mine;
	memset(&mine, 0, sizeof mine);
	{
		MapOut B;
		CHECK(map_alloc(B.g, nullptr, 2, 1, 1, 1, false) == LSFM_OK);
		fill(B.g);
		const int* stno = B.g.stno;
		B.give(&mine);
		CHECK(zeroed(B.g) && mine.stno == stno && mine.m == 2 && mine.n == 1);
	}
	CHECK(mine.stno[6 * 2 + 3 * 1 - 1] == 14 && mine.V[8] == 3.0); // (still readable: not freed with B)
	lsfm_map_release(&mine);
	lsfm_map_release(&mine);
	lsfm_map_release(nullptr);
	// a map without features: the index arrays alone, and no value array where none is asked for
	{
		MapOut C;
		CHECK(map_alloc(C.g, nullptr, 2, 0, 1, 0, false) == LSFM_OK);
		fill(C.g);
		const HostSystem h = host_system_of(C.g, false);
		CHECK(h.m == 2 && h.n == 0 && h.nU == 1 && h.nW == 0 && h.Ui == C.g.Ui && h.Uj == C.g.Uj && !h.U && !h.W && !h.V);
		std::vector<int> fptr;
		const char* why = nullptr;
		CHECK(system_check(h, false, fptr, &why) == LSFM_OK && fptr.size() == 1 && fptr[0] == 0);
	}
	printf("sanitize_map: ok (%d maps)\n", made);
	return 0;
}
