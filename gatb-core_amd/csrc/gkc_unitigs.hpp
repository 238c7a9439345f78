// gkc_unitigs.hpp — what gkc_unitigs.hip (the build), gkc_unitig_links.hip (the link CSR) and gkc_simplify.hip (tips, bulges, erroneous connections) share, and what
// gkc_paths.hip needs of them. Internal to the library.
#pragma once
#include "gkc_graph.hpp"

// records of unitig u, from the placement's first[] (n_alive: the records placed, all of them unless the placement was built over an alive array)
__device__ __forceinline__ uint64_t ut_length(const uint64_t* __restrict__ first, uint64_t n_alive, uint64_t n_unitigs, uint64_t u) { return (u + 1 < n_unitigs ? first[u + 1] : n_alive) - first[u]; }

// ------------------------------------------------------------------------------------------------ host side (gkc_unitigs.hip)
// q_prepare, then: the context holds a placement and it describes the results the context holds now (GKC_ERR_ARG otherwise)
int ut_require_placement(gkc_ctx* c, const char* who);
// The build behind gkc_graph_unitigs_build (d_alive == NULL: every record) and gkc_graph_unitigs_build_alive / the rounds of gkc_simplify.hip (the records with alive[i] != 0,
// n_alive of them; d_masks consistent with it: a dead record has mask 0 and no mask names it). q_prepare has run.
int ut_build(gkc_ctx* c, const char* who, const uint8_t* d_masks, const uint8_t* d_alive, uint64_t n_alive, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles);
// how many records of d_alive[0, n) are alive; with d_masks, *bad when a dead record has a mask. d_cnt16: 16 bytes of scratch; synchronised on return, also after a failure
int ut_alive_count(gkc_ctx* c, void* d_cnt16, const uint8_t* d_alive, const uint8_t* d_masks, uint64_t n, uint64_t* n_alive, bool* bad);
// ------------------------------------------------------------------------------------------------ host side (gkc_unitig_links.hip)
// gkc_graph_unitigs_links behind its guards. d_keep_slots (the rounds of gkc_simplify.hip; u32[2 n_unitigs] or NULL): where the record << 1 | end of every slot stays for the caller
int ut_links(gkc_ctx* c, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs, uint64_t* d_links, uint64_t cap_links, uint64_t* n_links, uint32_t* d_keep_slots);
