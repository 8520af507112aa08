// Merging feature pairs of a map: classes, output order and source lists from index arrays and the pairs alone
// (lsfm_merge_structure.hpp).  Plain C++: no device, no HIP header.
#include "lsfm_merge_structure.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "../../include/lsfm.h"
#include "lsfm_system.hpp"

namespace lsfm {

int merge_structure(int n, const std::vector<int>& fptr, const int* photo, const int* pairs, int K, MergeStructure& st, std::string& why)
{
	if (K < 1 || !pairs) { why = "no pairs: K < 1 or pairs is NULL"; return LSFM_ERR_ARG; }
	// ---- classes: union-find, the root of a class is its smallest member ----
	std::vector<int> root((size_t)n);
	std::iota(root.begin(), root.end(), 0);
	auto find = [&](int f) {
		int r = f;
		while (root[r] != r) r = root[r];
		while (root[f] != r) { const int up = root[f]; root[f] = r; f = up; }
		return r;
	};
	for (int a = 0; a < K; a++)
	{
		const int f = pairs[2 * a], g = pairs[2 * a + 1];
		if (f < 0 || f >= n || g < 0 || g >= n)
		{
			why = "pair " + std::to_string(a) + " (" + std::to_string(f) + ", " + std::to_string(g) + ") names a feature that is not one of the map's " + std::to_string(n);
			return LSFM_ERR_ARG;
		}
		if (f == g) { why = "pair " + std::to_string(a) + " names feature " + std::to_string(f) + " twice"; return LSFM_ERR_ARG; }
		const int rf = find(f), rg = find(g);
		if (rf != rg) root[std::max(rf, rg)] = std::min(rf, rg);
	}
	st = MergeStructure();
	st.n = n;
	st.rep.assign((size_t)n, 0);
	int no = 0;
	for (int f = 0; f < n; f++)
		if (find(f) == f) st.rep[f] = no++;
	for (int f = 0; f < n; f++) st.rep[f] = st.rep[find(f)];
	st.no = no; st.removed = n - no;
	// the members of every output feature, ascending (a counting sort keeps the order)
	st.cptr.assign((size_t)no + 1, 0);
	for (int f = 0; f < n; f++) st.cptr[st.rep[f] + 1]++;
	for (int c = 0; c < no; c++) st.cptr[c + 1] += st.cptr[c];
	st.cmem.assign((size_t)n, 0);
	{
		std::vector<int> at(st.cptr.begin(), st.cptr.end() - 1);
		for (int f = 0; f < n; f++) st.cmem[at[st.rep[f]]++] = f;
	}
	// ---- the output's W runs and their sources ----
	const int nW = fptr[n];
	st.photo.reserve(nW); st.feature.reserve(nW); st.sidx.reserve(nW);
	st.sptr.reserve((size_t)nW + 1);
	st.FBlock.assign((size_t)no + 1, 0);
	std::vector<int> blk; // the blocks of a class in (member, position) order
	for (int c = 0; c < no; c++)
	{
		st.FBlock[c] = (int)st.photo.size();
		const int m0 = st.cptr[c], m1 = st.cptr[c + 1];
		if (m1 - m0 == 1)
		{
			const int f = st.cmem[m0];
			for (int w = fptr[f]; w < fptr[f + 1]; w++)
			{
				st.sptr.push_back((int)st.sidx.size());
				st.sidx.push_back(w);
				st.photo.push_back(photo[w]); st.feature.push_back(c);
			}
			continue;
		}
		st.big++;
		st.bigs.push_back(c);
		blk.clear();
		for (int k = m0; k < m1; k++)
			for (int w = fptr[st.cmem[k]]; w < fptr[st.cmem[k] + 1]; w++) blk.push_back(w);
		std::stable_sort(blk.begin(), blk.end(), [&](int a, int b) { return photo[a] < photo[b]; });
		for (size_t i = 0; i < blk.size(); i++)
		{
			if (i == 0 || photo[blk[i]] != photo[blk[i - 1]])
			{
				st.sptr.push_back((int)st.sidx.size());
				st.photo.push_back(photo[blk[i]]); st.feature.push_back(c);
			}
			else if (i == 1 || photo[blk[i - 1]] != photo[blk[i - 2]]) st.multi++; // (the second source of an output block)
			st.sidx.push_back(blk[i]);
		}
	}
	st.nWo = (int)st.photo.size();
	st.FBlock[no] = st.nWo;
	st.sptr.push_back((int)st.sidx.size());
	return LSFM_OK;
}

} // namespace lsfm

extern "C" int lsfm_merge_structure(const lsfm_map* map, const int* pairs, int K, int* rep, int* photo, int* feature, int* FBlock, int* sptr, int* sidx,
                                    int cap_w, int* info, char* why, int why_cap)
{
	using namespace lsfm;
	auto fail = [&](const std::string& msg) {
		if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "%s", msg.c_str());
		return (int)LSFM_ERR_ARG;
	};
	if (why && why_cap > 0) why[0] = 0;
	if (!map) return fail("map is NULL");
	std::vector<int> fptr;
	const char* bad = nullptr;
	if (system_check(host_system_of(*map, false), false, fptr, &bad) != LSFM_OK) return fail(bad ? bad : "malformed map");
	MergeStructure st;
	std::string msg;
	if (merge_structure(map->n, fptr, map->photo, pairs, K, st, msg) != LSFM_OK) return fail(msg);
	if (info)
	{
		memset(info, 0, 8 * sizeof(int));
		info[0] = st.no; info[1] = st.nWo; info[2] = st.big; info[3] = st.removed; info[4] = st.multi;
	}
	if ((photo || feature || sptr) && cap_w < st.nWo) return fail("cap_w is too small: " + std::to_string(st.nWo) + " output blocks");
	if (sidx && cap_w < map->nW) return fail("cap_w is too small: " + std::to_string(map->nW) + " sources");
	auto put = [](int* dst, const std::vector<int>& v, size_t count) { if (dst && count) memcpy(dst, v.data(), count * sizeof(int)); };
	put(rep, st.rep, (size_t)st.n);
	put(photo, st.photo, (size_t)st.nWo);
	put(feature, st.feature, (size_t)st.nWo);
	put(FBlock, st.FBlock, (size_t)st.no);
	put(sptr, st.sptr, (size_t)st.nWo + 1);
	put(sidx, st.sidx, st.sidx.size());
	return LSFM_OK;
}
