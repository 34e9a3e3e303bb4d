// vss_build_info.cpp — the build's source stamp (include/vss.h vss_source_hash).
// VSS_STAMP_HASH is the first 16 hex digits of sha256 over the files of the Makefile's STAMPED line, in that line's
// order, computed at build time.  The Python loader (vss_amd/_native.py) recomputes the hash from the tree and refuses
// a library built from other sources, so a stale prebuilt .so can never be the one that runs.
#include "../../include/vss.h"

#ifndef VSS_STAMP_HASH
#error "VSS_STAMP_HASH must be defined by the build (csrc/Makefile)"
#endif

extern "C" const char* vss_source_hash(void) { return VSS_STAMP_HASH; }
