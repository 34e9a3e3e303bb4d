// vss_build_info.cpp — a library's source stamp: vss_source_hash (include/vss.h), vss_actuate_source_hash
// (include/vss_actuate.h) and vss_estimate_source_hash (include/vss_estimate.h), one compilation per library.
// VSS_STAMP_HASH is the first 16 hex digits of sha256 over the files of the library's Makefile's STAMPED line, in
// that line's order, computed at build time (stamped.mk); VSS_STAMP_FN is the function's name.  The Python loader
// (vss_amd/_native.py load_stamped) recomputes the hash from the tree and refuses a library built from other sources,
// so a stale prebuilt .so can never be the one that runs.
#if !defined(VSS_STAMP_HASH) || !defined(VSS_STAMP_FN)
#error "VSS_STAMP_HASH and VSS_STAMP_FN must be defined by the build (csrc/stamped.mk)"
#endif

extern "C" const char* VSS_STAMP_FN(void) { return VSS_STAMP_HASH; }
