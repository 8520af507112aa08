// Summing blocks into their places by source lists: the one kernel lsfm_gn_linearise (lsfm_gn.hip) and lsfm_map_merge_features
// (lsfm_merge.hip) share.
#pragma once
#include "lsfm_device.hpp"

namespace lsfm {

// Output block o is the sum of its sources sidx[sptr[o] .. sptr[o + 1]) in that order (at least one).  One lane per output block,
// consecutive lanes on consecutive output blocks; the sources of neighbouring output blocks lie in the same feature's run (or the
// runs of one class of features).  The sum is held in registers and stored once.  No atomics: given the sources the result is the
// same bits every time.  HBM-bound: 8 N bytes per source in, 8 N bytes per output block out (W: 144 B, U: 288 B), no products.
template <int N>
__global__ void __launch_bounds__(256)
k_gn_coalesce(int no, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ src, double* __restrict__ dst)
{
	const int o = blockIdx.x * blockDim.x + threadIdx.x;
	if (o >= no) return;
	double acc[N], v[N];
	const int q0 = sptr[o], q1 = sptr[o + 1];
	ld<N>(acc, src + (size_t)sidx[q0] * N);
	for (int q = q0 + 1; q < q1; q++)
	{
		ld<N>(v, src + (size_t)sidx[q] * N);
#pragma unroll
		for (int i = 0; i < N; i++) acc[i] += v[i];
	}
	st<N>(dst + (size_t)o * N, acc);
}

} // namespace lsfm
