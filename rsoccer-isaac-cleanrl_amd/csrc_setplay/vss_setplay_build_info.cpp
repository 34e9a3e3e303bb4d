// vss_setplay_build_info.cpp — the unit's source stamp (include/vss_setplay.h vss_setplay_source_hash).
// VSS_SETPLAY_STAMP_HASH is the first 16 hex digits of sha256 over the files of this directory's Makefile's STAMPED
// line, in that line's order, computed at build time.  The Python loader (vss_amd/setplay.py) recomputes the hash from
// the tree and refuses a library built from other sources, so a stale prebuilt .so can never be the one that runs.
#include "../../include/vss_setplay.h"

#ifndef VSS_SETPLAY_STAMP_HASH
#error "VSS_SETPLAY_STAMP_HASH must be defined by the build (csrc_setplay/Makefile)"
#endif

extern "C" const char* vss_setplay_source_hash(void) { return VSS_SETPLAY_STAMP_HASH; }
