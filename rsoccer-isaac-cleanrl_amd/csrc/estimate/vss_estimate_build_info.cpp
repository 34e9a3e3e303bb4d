// vss_estimate_build_info.cpp — the source stamp of libvss_estimate.so (include/vss_estimate.h vss_estimate_source_hash).
// VSS_ESTIMATE_SOURCE_HASH is the first 16 hex digits of sha256 over the files of this directory's Makefile's STAMPED
// line, in its order, computed at build time; vss_amd/estimate.py recomputes it from the tree and refuses a library
// built from other sources, as vss_amd/actuate.py does for its own.
#include "../../../include/vss_estimate.h"

#ifndef VSS_ESTIMATE_SOURCE_HASH
#error "VSS_ESTIMATE_SOURCE_HASH must be defined by the build (csrc/estimate/Makefile)"
#endif

extern "C" const char* vss_estimate_source_hash(void) { return VSS_ESTIMATE_SOURCE_HASH; }
