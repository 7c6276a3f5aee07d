# oracle/integration.mk — TEST INFRASTRUCTURE ONLY. Included by oracle/Makefile
# (REF and CXX come from there); `make -C oracle integration`, after the
# product library (`make lib` in the repository root) and the `ref` target.
#
# Builds the transport decorator and the drop-in harnesses of integration/
# against the reference tree, where that tree is present. Whatever is
# compiled from the reference goes under oracle/_ref/ (git-ignored), beside
# _ref/libtulips_ref.so: that folder is the one place reference-built
# binaries live, so a machine without the reference tree that is handed
# oracle/_ref/ can still run tests/test_gpucsum_device.py and
# tests/test_dropin.py.
#
#   _ref/integration/libgpucsum_test.so
#                               gpucsum::Device (ours) + test/gpucsum_harness
#                               (ours) + the reference's list::Device, linked
#                               to _ref/libtulips_ref.so (the reference's
#                               stack/system build) and to
#                               tulips_amd/libtulips_csum.so (the product).
#
# In the reference tree the decorator is built by
# src/transport/gpucsum/CMakeLists.txt instead.

ROOT := $(abspath ..)
INT := $(ROOT)/integration
B := _ref/integration
CXXFLAGS_INT = -std=c++17 -O2 -fPIC -Wall -Wextra -Wno-unused-parameter \
           -Wno-address-of-packed-member \
           -I$(INT)/include -I$(REF)/include -I$(ROOT)/include

OUT = $(B)/libgpucsum_test.so
SRCS = $(INT)/src/transport/gpucsum/Device.cpp $(INT)/test/gpucsum_harness.cpp \
       $(REF)/src/transport/list/Device.cpp

.PHONY: integration dropin

integration: $(OUT) dropin

$(OUT): $(SRCS) $(INT)/include/tulips/transport/gpucsum/Device.h $(ROOT)/include/tulips_csum.h \
        $(ROOT)/tulips_amd/libtulips_csum.so _ref/libtulips_ref.so
	@mkdir -p $(B)
	$(CXX) $(CXXFLAGS_INT) -shared -o $@ $(SRCS) \
	    -L$(ROOT)/tulips_amd -ltulips_csum -L_ref -ltulips_ref \
	    -Wl,-rpath,'$$ORIGIN/../../../tulips_amd' -Wl,-rpath,'$$ORIGIN/..' \
	    -lpthread

# ---------------------------------------------------------------------------
# dropin: the product linked into the reference's own stack (DESIGN.md §1,
# INTEGRATION.md §1). The reference's unmodified src/stack + src/system +
# src/api + src/transport/list sources are compiled where they lie, with the
# reference's release flags (-O3 -mssse3, -fPIC as its shared libtulips_stack,
# src/stack/CMakeLists.txt:7-9), once per gate variant:
#   default  checks and generation in the stack (the reference default)
#   nocheck  -DTULIPS_DISABLE_CHECKSUM_CHECK (receive checks left to the
#            device: the gpucsum decorator)
#   offload  + -DTULIPS_HAS_HW_CHECKSUM (generation left to the device too)
# (CMakeLists.txt:46-47,151-163; ARP and ICMP enabled as the reference's
# tests build them). integration/strip_checksums.sh then removes the
# reference's checksum definitions from those objects, the objects become
# _ref/integration/dropin/<v>/libtulips_stack_dropin.so (NEEDing
# libtulips_csum.so), and integration/test/dropin_harness.cpp + the gpucsum
# decorator link against libtulips_csum.so FIRST, then that stack.
DROPIN_VARIANTS = default nocheck offload
DEFS_default = -DTULIPS_ENABLE_ARP -DTULIPS_ENABLE_ICMP -DTULIPS_CLOCK_HAS_OFFSET
DEFS_nocheck = $(DEFS_default) -DTULIPS_DISABLE_CHECKSUM_CHECK
DEFS_offload = $(DEFS_nocheck) -DTULIPS_HAS_HW_CHECKSUM
DROPIN_CXXFLAGS = -std=c++17 -O3 -mssse3 -fPIC -w -I$(REF)/include
DROPIN_SRCS = $(wildcard $(REF)/src/stack/*.cpp) \
              $(wildcard $(REF)/src/stack/arp/*.cpp) \
              $(REF)/src/stack/arp/stubs/linux.cpp \
              $(wildcard $(REF)/src/stack/ethernet/*.cpp) \
              $(wildcard $(REF)/src/stack/ipv4/*.cpp) \
              $(wildcard $(REF)/src/stack/icmpv4/*.cpp) \
              $(wildcard $(REF)/src/stack/tcpv4/*.cpp) \
              $(wildcard $(REF)/src/system/*.cpp) \
              $(wildcard $(REF)/src/api/*.cpp) \
              $(REF)/src/transport/list/Device.cpp

dropin: $(foreach v,$(DROPIN_VARIANTS),$(B)/dropin/$(v)/dropin_harness)

define DROPIN_VARIANT
$(B)/dropin/$(1)/obj/%.o: $(REF)/src/%.cpp
	@mkdir -p $$(dir $$@)
	$(CXX) $(DROPIN_CXXFLAGS) $(DEFS_$(1)) -c $$< -o $$@

$(B)/dropin/$(1)/stripped.txt: $(patsubst $(REF)/src/%.cpp,$(B)/dropin/$(1)/obj/%.o,$(DROPIN_SRCS)) $(INT)/strip_checksums.sh
	$(INT)/strip_checksums.sh $(B)/dropin/$(1)/obj > $$@

$(B)/dropin/$(1)/libtulips_stack_dropin.so: $(B)/dropin/$(1)/stripped.txt $(ROOT)/tulips_amd/libtulips_csum.so
	$(CXX) -shared -o $$@ $(patsubst $(REF)/src/%.cpp,$(B)/dropin/$(1)/obj/%.o,$(DROPIN_SRCS)) \
	    -Wl,--no-as-needed -L$(ROOT)/tulips_amd -ltulips_csum \
	    -Wl,-rpath,'$$$$ORIGIN/../../../../../tulips_amd' -lpthread

$(B)/dropin/$(1)/dropin_harness: $(INT)/test/dropin_harness.cpp $(INT)/src/transport/gpucsum/Device.cpp \
        $(INT)/include/tulips/transport/gpucsum/Device.h $(ROOT)/include/tulips_csum.h \
        $(B)/dropin/$(1)/libtulips_stack_dropin.so
	$(CXX) -std=c++17 -O2 -w -I$(INT)/include -I$(REF)/include -I$(ROOT)/include $(DEFS_$(1)) \
	    -DDROPIN_GPUCSUM -o $$@ $(INT)/test/dropin_harness.cpp $(INT)/src/transport/gpucsum/Device.cpp \
	    -Wl,--no-as-needed -L$(ROOT)/tulips_amd -ltulips_csum \
	    -L$(B)/dropin/$(1) -ltulips_stack_dropin \
	    -Wl,-rpath,'$$$$ORIGIN' -Wl,-rpath,'$$$$ORIGIN/../../../../../tulips_amd' -ldl -lpthread
endef
$(foreach v,$(DROPIN_VARIANTS),$(eval $(call DROPIN_VARIANT,$(v))))
