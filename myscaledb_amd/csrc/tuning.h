// tuning.h -- A/B switches for measurement builds only.
//
// The release library (libmqvs.so) never reads the environment: every switch
// below returns its default there, so no variable in a server's environment
// can change a kernel or select a diagnostic build.  The measurement build
// (`make dbg` -> libmqvs_dbg.so, compiled with -DMQVS_DEBUG_TUNING) reads
// them with getenv; tools load it only through an explicit
// myscaledb_amd._lib.use_measurement_build() call (their --dbg option).
//
// Every switch only forces a path, or sets a number, that the release build
// reaches under its own conditions: none selects a kernel build of its own.
// Both libraries therefore hold the same list of kernels, and the measurement
// build differs only in reading the environment (and in k_coarse_pick
// carrying its MQVS_PICK_TRACE timestamps).  Variants that lost their A/B are
// deleted, not switched off: DESIGN.md "Retired variants" lists them.
//
// The switches (this table is the whole list):
//
//   name                 default       what it forces                         read in
//   MQVS_SEG             per nq        "first,growth,target" of the search's  search.hip seg_tune
//                                      row segments
//   MQVS_P4_ORD          1             0: no cosine ordinal planes (each      search.hip FlatSearch
//                                      lane picks its query's variant)
//   MQVS_P4_MAP          1             0: tile sequence x + 8 tg (a kernel    kernels_p4.hip launch_p4_any
//                                      argument of k_scan_p4m)
//   MQVS_HI_PP           2             != 2: batches skip the batch kernel    kernels_hi.hip launch_hi_t
//                                      and take k_scan_hi
//   MQVS_HI_REG          1             0: small batches take k_scan_hi, not   kernels_hi.hip launch_hi_t,
//                                      k_scan_hi_reg                          scan_hi_small_tiles_ok
//   MQVS_HI_SMALL_TILES  1             0: no kBfRowsSmall-row tiles           kernels_hi.hip scan_hi_small_tiles_ok
//   MQVS_HI_SMALL_MAIN   1             0: small tiles for probe scans only    search.hip FlatSearch
//   MQVS_IVF_QG          by pairs per  queries per list-scan group: 16, 32,   index.hip list_pass
//                        list          64
//   MQVS_IVF_CHUNK       8 qg          rows per list-scan work item           index.hip list_pass
//   MQVS_IVF_GRID        4096          workgroups of the list scan            index.hip list_pass
//   MQVS_IVF_PAIR        1             0: the planned list scan where the     index.hip list_pass
//                                      pair-mode scan would run
//   MQVS_IVF_COARSE      2 (else by    coarse step: 2 pick, 1 FLAT search of  index.hip search_index_impl
//                        nlist)        the centroids, 0 list pass
//   MQVS_PICK_TRACE      0             1: k_coarse_pick prints phase          kernels_ivf_pick.hip launch_coarse_pick
//                                      timestamps of three workgroups
//   MQVS_RR_1W_NQ        16            largest nq of k_exact_records_1w       kernels_rerank.hip launch_exact_rerank
//   MQVS_BIN_GRID        4096          workgroup cap of the binary scan       kernels_binary.hip
//   MQVS_BIN_NOCO        unset         set: small binary batches skip         kernels_binary.hip
//                                      k_scan_binary_co
#pragma once

#include <cstdlib>

namespace mqvs {

#ifdef MQVS_DEBUG_TUNING
constexpr bool kDebugTuning = true;
inline const char *tune_env(const char *name) { return std::getenv(name); }
#else
constexpr bool kDebugTuning = false;
inline const char *tune_env(const char *) { return nullptr; }
#endif

// integer switch: the variable's value in a measurement build, dflt otherwise
inline int tune_int(const char *name, int dflt) {
    const char *e = tune_env(name);
    return (e && *e) ? std::atoi(e) : dflt;
}

}  // namespace mqvs
