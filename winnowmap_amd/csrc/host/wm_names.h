// wm_names.h — contig names as integers, for the self / all-vs-all switches -D, --dual=no, -X.
// skip_seed (src/map.c:132-154) compares the query's name with the name of every contig it hits (strcmp). Strings do not go to the device; integers do:
// rank[rid] = dense rank of contig rid's name among the DISTINCT contig names in strcmp order (contigs that share a name share a rank), sorted[r] = a contig
// that carries the name of rank r. A query name becomes the key (lo, eq): lo = distinct contig names that are smaller, eq = the name occurs among the
// contigs (one binary search per read, not per anchor). Then
//   strcmp(qname, name[rid]) == 0  <=>  eq && rank[rid] == lo          strcmp(qname, name[rid]) > 0  <=>  rank[rid] < lo
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>

namespace wm {

struct NameTable { std::vector<uint32_t> rank, sorted; };
struct NameKey { uint32_t lo = 0, eq = 0; };

// name_of(i): the C string of contig i
template <class NameOf> NameTable rank_names(size_t n, NameOf name_of)
{
	NameTable t;
	std::vector<uint32_t> ord(n);
	for (size_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
	std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { const int c = strcmp(name_of(a), name_of(b)); return c != 0 ? c < 0 : a < b; });
	t.rank.resize(n);
	for (size_t i = 0; i < n; ++i) {
		if (i == 0 || strcmp(name_of(ord[i - 1]), name_of(ord[i])) != 0) t.sorted.push_back(ord[i]);
		t.rank[ord[i]] = (uint32_t)t.sorted.size() - 1;
	}
	return t;
}

template <class NameOf> NameKey name_key(const NameTable &t, NameOf name_of, const char *qname)
{
	NameKey k;
	size_t lo = 0, hi = t.sorted.size();
	while (lo < hi) {                                                  // the first distinct contig name that is not smaller than qname
		const size_t mid = (lo + hi) >> 1;
		if (strcmp(name_of(t.sorted[mid]), qname) < 0) lo = mid + 1; else hi = mid;
	}
	k.lo = (uint32_t)lo;
	k.eq = lo < t.sorted.size() && strcmp(name_of(t.sorted[lo]), qname) == 0;
	return k;
}

} // namespace wm
