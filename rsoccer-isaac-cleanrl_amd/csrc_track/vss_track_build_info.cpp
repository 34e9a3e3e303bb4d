// vss_track_build_info.cpp — the unit's source stamp (include/vss_track.h vss_track_source_hash).
// VSS_TRACK_STAMP_HASH is the first 16 hex digits of sha256 over the files of this directory's Makefile's STAMPED
// line, in that line's order, computed at build time.  The Python loader (vss_amd/track.py) recomputes the hash from
// the tree and refuses a library built from other sources, so a stale prebuilt .so can never be the one that runs.
#include "../../include/vss_track.h"

#ifndef VSS_TRACK_STAMP_HASH
#error "VSS_TRACK_STAMP_HASH must be defined by the build (csrc_track/Makefile)"
#endif

extern "C" const char* vss_track_source_hash(void) { return VSS_TRACK_STAMP_HASH; }
