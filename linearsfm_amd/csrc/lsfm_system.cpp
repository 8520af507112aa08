// The index arrays of a system from host arrays, checked on the host (lsfm_system.hpp).  Plain C++: no device, no HIP header.
#include "lsfm_system.hpp"

#include "../../include/lsfm.h"

namespace lsfm {

int system_check(const HostSystem& h, bool empty_features_ok, std::vector<int>& fptr, const char** why)
{
	auto fail = [&](const char* msg) { if (why) *why = msg; return (int)LSFM_ERR_ARG; };
	if (h.m < 0 || h.n < 0 || h.nU < 0 || h.nW < 0) return fail("negative map size");
	if ((h.nU && (!h.Ui || !h.Uj)) || (h.nW && (!h.photo || !h.feature))) return fail("null index array");
	fptr.assign((size_t)h.n + 1, 0);
	int j = 0;
	for (int f = 0; f < h.n; f++)
	{
		fptr[f] = j;
		while (j < h.nW && h.feature[j] == f) j++;
		if (j == fptr[f] && !empty_features_ok) return fail("every feature needs at least one W block, W sorted by feature");
	}
	if (j != h.nW) return fail("W is not sorted by feature");
	fptr[h.n] = h.nW;
	for (int i = 0; i < h.nU; i++)
		if (h.Ui[i] < 0 || h.Uj[i] >= h.m || h.Ui[i] > h.Uj[i]) return fail("U block coordinates must satisfy 0 <= Ui <= Uj < m");
	for (int k = 0; k < h.nW; k++)
		if (h.photo[k] < 0 || h.photo[k] >= h.m) return fail("photo index out of range");
	return LSFM_OK;
}

std::vector<unsigned char> gauge_mask(int m, int blk, int scalar)
{
	std::vector<unsigned char> fx((size_t)m * 6, 0);
	if (blk >= 0 && blk < m) for (int i = 0; i < 6; i++) fx[(size_t)blk * 6 + i] = 1;
	if (scalar >= 0 && scalar < 6 * m) fx[scalar] = 1;
	return fx;
}

} // namespace lsfm
