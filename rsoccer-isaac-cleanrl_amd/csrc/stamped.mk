# The build rules of a stamped library, once, for csrc/Makefile, actuate/Makefile and estimate/Makefile.  The
# including Makefile names its default goal and sets, before the include:
#   STAMPED          every file the library is built from (its own literal line: vss_amd/_native.py reads it); a
#                    translation unit is written <source>:<its flag set>; this fragment is one of the files
#   STAMP_LIB        the library to link, STAMP_OBJ the directory of its objects
#   STAMP_FN         the exported function that returns the source stamp
#   SOME_UNITS_ONLY  stamped headers that only some units include (those objects name the .sha themselves)
# The source stamp is the sha256 of the STAMPED files in that line's order, compiled into vss_build_info.cpp.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
FILES := $(foreach w,$(STAMPED),$(firstword $(subst :, ,$w)))
UNITS := $(basename $(filter %.hip,$(FILES)))
flags = $($(patsubst $1.hip:%,%,$(filter $1.hip:%,$(STAMPED))))
# resource-usage reports the units with a flag set of their own: their registers and scratch are what the flags are for
REPORTED := $(basename $(filter %.hip,$(subst :, ,$(filter-out %:COMMON,$(STAMPED)))))
SRC_HASH := $(shell cat $(FILES) | sha256sum | cut -c1-16)
COMMON := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall
STEP_FLAGS := $(COMMON) -ffp-contract=off
BUILD_INFO := $(dir $(lastword $(MAKEFILE_LIST)))vss_build_info.cpp

# Rebuilds are content-based, not mtime-based: each source's sha256 is kept in $(STAMP_OBJ)/<file>.sha, rewritten
# (and so made newer than the objects) only when the content changes; objects depend on those files.
define content_stamp
@mkdir -p $(STAMP_OBJ); h=$$(sha256sum $< | cut -c1-64); [ "$$(cat $@ 2>/dev/null)" = "$$h" ] || echo "$$h" > $@
endef
sha = $(patsubst %,$(STAMP_OBJ)/%.sha,$(notdir $1))
define sha_rule
$(call sha,$1): $1 FORCE ; $$(content_stamp)
endef
$(foreach f,$(FILES) $(BUILD_INFO),$(eval $(call sha_rule,$f)))

# every unit depends on its source and on every stamped file that is not a unit, but for the SOME_UNITS_ONLY headers
$(UNITS:%=$(STAMP_OBJ)/%.o): $(STAMP_OBJ)/%.o: $(STAMP_OBJ)/%.hip.sha $(call sha,$(filter-out %.hip $(SOME_UNITS_ONLY),$(FILES)))
	mkdir -p $(STAMP_OBJ)
	$(HIPCC) $(call flags,$*) -c -o $@ $*.hip

$(STAMP_OBJ)/vss_build_info.o: $(call sha,$(BUILD_INFO) $(FILES))
	mkdir -p $(STAMP_OBJ)
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -DVSS_STAMP_FN=$(STAMP_FN) -DVSS_STAMP_HASH='"$(SRC_HASH)"' -c -o $@ $(BUILD_INFO)

$(STAMP_LIB): $(UNITS:%=$(STAMP_OBJ)/%.o) $(STAMP_OBJ)/vss_build_info.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

resource-usage: $(REPORTED:%=%.resource-usage)
%.resource-usage: %.hip
	$(HIPCC) $(call flags,$*) -Rpass-analysis=kernel-resource-usage -c -o /tmp/$*.ru.o $< 2>&1 | grep -E "Function Name|VGPRs:|AGPRs:|SGPRs:|Occupancy|LDS Size|ScratchSize"

clean:
	rm -rf $(STAMP_LIB) $(STAMP_OBJ)

FORCE:
.PHONY: all clean resource-usage FORCE
