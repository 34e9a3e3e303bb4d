// vss_referee_build_info.cpp — the unit's source stamp (include/vss_referee.h vss_referee_source_hash).
// VSS_REFEREE_STAMP_HASH is the first 16 hex digits of sha256 over the files of this directory's Makefile's STAMPED
// line, in that line's order, computed at build time.  The Python loader (vss_amd/referee.py) recomputes the hash from
// the tree and refuses a library built from other sources, so a stale prebuilt .so can never be the one that runs.
#include "../../include/vss_referee.h"

#ifndef VSS_REFEREE_STAMP_HASH
#error "VSS_REFEREE_STAMP_HASH must be defined by the build (csrc_referee/Makefile)"
#endif

extern "C" const char* vss_referee_source_hash(void) { return VSS_REFEREE_STAMP_HASH; }
