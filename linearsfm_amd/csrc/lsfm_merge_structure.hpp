// Merging feature pairs of a map (lsfm_map_merge_features), the part that depends on index arrays and the pairs alone: the classes of
// the pair graph, the output's feature order and W runs, and per output W block its sources.  Plain C++ (lsfm_merge_structure.cpp,
// compiled by g++ like lsfm_gn_structure.cpp: callable without a device; C ABI: lsfm_merge_structure); the numbers are lsfm_merge.hip.
#pragma once
#include <string>
#include <vector>

struct lsfm_map;

namespace lsfm {

// A class = a connected component of the pair graph; its representative is its member with the smallest index; output feature c is
// the c-th representative in ascending order (an untouched feature is a class of one).
struct MergeStructure {
	int n = 0, no = 0, nWo = 0;      // input features; output features n', output W blocks nW'
	int big = 0, removed = 0, multi = 0; // classes of more than one member; features removed (n - n'); output blocks with more than one source
	std::vector<int> rep;            // [n] output feature of every input feature
	std::vector<int> cptr, cmem;     // [n' + 1] / [n] the members of every output feature, ascending
	std::vector<int> photo, feature; // [nW'] output W: sorted by feature; a class of one keeps its run as it stands (repeated blocks
	                                 // stay), a larger class has one block per pose, ascending
	std::vector<int> FBlock;         // [n' + 1] first output block of every output feature (entry n': nW')
	std::vector<int> sptr, sidx;     // [nW' + 1] / [nW] the sources of an output block (input W blocks), by (member, position in the input)
	std::vector<int> bigs;           // [big] the output features with more than one member, ascending
};

// fptr[n + 1]: the W runs of the input's features (system_check).  LSFM_OK, or LSFM_ERR_ARG with `why`: K < 1, an index out of range,
// f == g.  A pair given twice, in either order, and a pair that closes a cycle are fine.
int merge_structure(int n, const std::vector<int>& fptr, const int* photo, const int* pairs, int K, MergeStructure& st, std::string& why);

} // namespace lsfm
