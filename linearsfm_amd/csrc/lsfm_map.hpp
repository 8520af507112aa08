// The maps the library itself makes (lsfm_map.cpp): their one allocator, its counterpart lsfm_map_release, and an owner for the
// stretch between the two.  Plain C++ (compiled by g++ like lsfm_system.cpp: callable without a device).
#pragma once
#include <cstring>

#include "../../include/lsfm.h"

namespace lsfm {

// g = a zeroed map of the given sizes with every array from the allocator lsfm_map_release frees (pose_origin [m] where asked for), and
// Ref, FRef, ScaP, Fix, Sign, FScaP, FFix of `like` (null: zeros).  LSFM_OK, or LSFM_ERR_OOM with g zeroed and nothing held.
int map_alloc(lsfm_map& g, const lsfm_map* like, int m, int n, int nU, int nW, bool pose_origin);

// a library-made map until it is the caller's: released on every way out that does not give() it
struct MapOut {
	lsfm_map g;
	MapOut() { memset(&g, 0, sizeof g); }
	~MapOut() { lsfm_map_release(&g); }
	MapOut(const MapOut&) = delete;
	MapOut& operator=(const MapOut&) = delete;
	void give(lsfm_map* out) { *out = g; memset(&g, 0, sizeof g); }
};

} // namespace lsfm
