# wave testbench (TEST INFRASTRUCTURE): what the Makefiles of tests/emu, tests/emu_clips and tests/emu_push share — the HIP kernel source compiled for the
# host with 64 fibres per wavefront, no sanitizer (the libraries are loaded into Python).  A library depends on every kernel header, so a new one cannot leave
# a stale library behind.
CXX ?= g++
CSRC = ../../deepmimic_mujoco_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -std=c++17 -DDM_WAVE_TESTBENCH -I../emu -I$(CSRC) -I../../include -ffp-contract=off -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas
TESTBENCH_DEPS = ../emu/emu_main.cpp ../emu/wave_testbench.h ../emu/wave_fibres.h ../emu/host_batch.h ../emu/testbench.mk $(wildcard $(CSRC)/*.h) ../../include/dmenv.h
