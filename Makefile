# Top-level convenience targets. The product is built by `python -m acvm_amd.build` (hipcc, gfx950); the oracle by oracle/Makefile.
#   make asan   the host code that parses untrusted bytes (circuit reader, WitnessMap reader, planner) with AddressSanitizer and
#               UndefinedBehaviorSanitizer, CPU only: tools/asan/fuzz_driver (tests/test_fuzz_reader.py feeds it mutated circuits), and the
#               checks of the device imports' descriptors, parts and lists: tools/asan/import_plan_host_test (tests/test_import_plan_on_host.py
#               feeds it its command streams), and the assigned set of the host reads: tools/asan/assigned_view_host_test
#               (tests/test_assigned_view_on_host.py), and the checks and tile views of the node's device form: tools/asan/node_io_plan_host_test
#               (tests/test_node_io_plan_on_host.py), and the site lists, refusals, shapes and capacity rule of the batch-wide foreign calls:
#               tools/asan/foreign_plan_host_test (tests/test_foreign_plan_on_host.py), and their per-row form -- the lanes a mask resumes, the
#               refusal order, the width behind the sizing launch: tools/asan/foreign_rows_plan_host_test -- with the per-row append of the result
#               store run on the host: tools/asan/foreign_rows_store_host_test (hipcc, host side sanitized; tests/test_foreign_rows_on_host.py), and the
#               host-only decisions of the node's foreign-call loop -- handler checks, row_base, scratch sizes, round cap:
#               tools/asan/node_foreign_plan_host_test (tests/test_foreign_rows_on_host.py), and the masked import's addressing arithmetic and
#               plan: tools/asan/import_mask_host_test (hipcc, host side sanitized; tests/test_import_mask_on_host.py), and the checks, field table and
#               window cut of the record import: tools/asan/record_plan_host_test (tests/test_record_plan_on_host.py), and the checks, window cut,
#               cover bitmaps and field table of the record export: tools/asan/record_out_plan_host_test (tests/test_record_out_plan_on_host.py), and the
#               checks, unit placement and tables of the masked record import: tools/asan/record_mask_plan_host_test
#               (tests/test_record_mask_plan_on_host.py), and the checks, ranks, bound and CRC power table of the batch-wide wire format:
#               tools/asan/wire_plan_host_test (tests/test_wire_plan_on_host.py), and the checks, key table and row judgement of the batch-wide
#               wire import: tools/asan/wire_in_plan_host_test (tests/test_wire_in_plan_on_host.py), and the code tables, constant header and
#               bound of its deflating container: tools/asan/wire_deflate_plan_host_test (tests/test_wire_deflate_plan_on_host.py), and the
#               gzip import: its checks, arena layout and fixed-code tables: tools/asan/wire_inflate_plan_host_test
#               (tests/test_wire_inflate_plan_on_host.py), and the per-row inflater the kernel runs, on the host over untrusted rows in heap blocks
#               of exactly their bounds: tools/asan/wire_inflate_host_test (hipcc, host side sanitized; tests/test_wire_inflate_on_host.py), and the
#               decisions of the Brillig retry loop -- continue, restart or final, the next pass's limits, columns and bytes:
#               tools/asan/brillig_retry_plan_host_test (tests/test_brillig_retry_plan_on_host.py), and the checkpoint record, the scratch's index
#               functions and the relocation run on host arrays of exactly their sizes: tools/asan/brillig_resume_host_test (hipcc, host side
#               sanitized; tests/test_brillig_resume_on_host.py), and the packed wire export's checks, chunk rule, arena carve and capacity rule:
#               tools/asan/wire_pack_plan_host_test (tests/test_wire_pack_plan_on_host.py), and the repitch kernel's per-lane body, the scan's block
#               arithmetic and the offsets judgement on heap blocks of exactly the stated sizes: tools/asan/wire_repitch_host_test (hipcc, host
#               side sanitized; tests/test_wire_pack_on_host.py)
CXX ?= g++
ASAN_FLAGS = -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-sign-compare
ASAN_SRCS = tools/asan/fuzz_driver.cpp acvm_amd/csrc/circuit.cpp acvm_amd/csrc/plan.cpp acvm_amd/csrc/tuning.cpp acvm_amd/csrc/schedule.cpp acvm_amd/csrc/schedule_check.cpp
PLAN_SRCS = tools/import_plan_host_test.cpp acvm_amd/csrc/import_plan.cpp
NODE_IO_SRCS = tools/node_io_plan_host_test.cpp acvm_amd/csrc/node_io_plan.cpp acvm_amd/csrc/import_plan.cpp
FOREIGN_SRCS = tools/foreign_plan_host_test.cpp acvm_amd/csrc/foreign_plan.cpp acvm_amd/csrc/import_plan.cpp
FOREIGN_ROWS_SRCS = tools/foreign_rows_plan_host_test.cpp acvm_amd/csrc/foreign_plan.cpp acvm_amd/csrc/import_plan.cpp
NODE_FOREIGN_SRCS = tools/node_foreign_plan_host_test.cpp acvm_amd/csrc/node_foreign_plan.cpp acvm_amd/csrc/import_plan.cpp
RECORD_SRCS = tools/record_plan_host_test.cpp acvm_amd/csrc/record_plan.cpp acvm_amd/csrc/import_plan.cpp
RECORD_MASK_SRCS = tools/record_mask_plan_host_test.cpp acvm_amd/csrc/record_plan.cpp acvm_amd/csrc/import_plan.cpp
RECORD_OUT_SRCS = tools/record_out_plan_host_test.cpp acvm_amd/csrc/record_out_plan.cpp acvm_amd/csrc/import_plan.cpp
WIRE_SRCS = tools/wire_plan_host_test.cpp acvm_amd/csrc/wire_plan.cpp
WIRE_DEFLATE_SRCS = tools/wire_deflate_plan_host_test.cpp acvm_amd/csrc/wire_plan.cpp
WIRE_IN_SRCS = tools/wire_in_plan_host_test.cpp acvm_amd/csrc/wire_in_plan.cpp acvm_amd/csrc/wire_plan.cpp
WIRE_INFLATE_PLAN_SRCS = acvm_amd/csrc/wire_inflate_plan.cpp acvm_amd/csrc/wire_in_plan.cpp acvm_amd/csrc/wire_plan.cpp
WIRE_INFLATE_HDRS = acvm_amd/csrc/wire_inflate_plan.hpp acvm_amd/csrc/wire_in_plan.hpp acvm_amd/csrc/wire_plan.hpp include/acvm_amd.h
HIPCC ?= /opt/rocm/bin/hipcc
asan: tools/asan/fuzz_driver tools/asan/import_plan_host_test tools/asan/assigned_view_host_test tools/asan/node_io_plan_host_test tools/asan/foreign_plan_host_test \
      tools/asan/foreign_rows_plan_host_test tools/asan/foreign_rows_store_host_test tools/asan/node_foreign_plan_host_test tools/asan/import_mask_host_test \
      tools/asan/record_plan_host_test tools/asan/record_out_plan_host_test tools/asan/record_mask_plan_host_test tools/asan/wire_plan_host_test \
      tools/asan/wire_in_plan_host_test tools/asan/wire_deflate_plan_host_test tools/asan/wire_inflate_plan_host_test tools/asan/wire_inflate_host_test \
      tools/asan/brillig_retry_plan_host_test tools/asan/brillig_resume_host_test tools/asan/wire_pack_plan_host_test tools/asan/wire_repitch_host_test
tools/asan/fuzz_driver: $(ASAN_SRCS) $(wildcard acvm_amd/csrc/*.hpp)
	$(CXX) $(ASAN_FLAGS) -o $@ $(ASAN_SRCS) -lz
tools/asan/import_plan_host_test: $(PLAN_SRCS) acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(PLAN_SRCS)
tools/asan/node_io_plan_host_test: $(NODE_IO_SRCS) acvm_amd/csrc/node_io_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(NODE_IO_SRCS)
tools/asan/foreign_plan_host_test: $(FOREIGN_SRCS) acvm_amd/csrc/foreign_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(FOREIGN_SRCS)
tools/asan/foreign_rows_plan_host_test: $(FOREIGN_ROWS_SRCS) acvm_amd/csrc/foreign_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(FOREIGN_ROWS_SRCS)
tools/asan/foreign_rows_store_host_test: tools/foreign_rows_store_host_test.hip acvm_amd/csrc/foreign_store.hpp
	$(HIPCC) --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tools/foreign_rows_store_host_test.hip
tools/asan/import_mask_host_test: tools/import_mask_host_test.hip acvm_amd/csrc/import_plan.cpp acvm_amd/csrc/import_mask.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(HIPCC) --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tools/import_mask_host_test.hip acvm_amd/csrc/import_plan.cpp
tools/asan/node_foreign_plan_host_test: $(NODE_FOREIGN_SRCS) acvm_amd/csrc/node_foreign_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(NODE_FOREIGN_SRCS)
tools/asan/record_plan_host_test: $(RECORD_SRCS) acvm_amd/csrc/record_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(RECORD_SRCS)
tools/asan/record_mask_plan_host_test: $(RECORD_MASK_SRCS) acvm_amd/csrc/record_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(RECORD_MASK_SRCS)
tools/asan/record_out_plan_host_test: $(RECORD_OUT_SRCS) acvm_amd/csrc/record_out_plan.hpp acvm_amd/csrc/record_plan.hpp acvm_amd/csrc/import_plan.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(RECORD_OUT_SRCS)
tools/asan/wire_plan_host_test: $(WIRE_SRCS) acvm_amd/csrc/wire_plan.hpp acvm_amd/csrc/assigned_view.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(WIRE_SRCS)
tools/asan/wire_deflate_plan_host_test: $(WIRE_DEFLATE_SRCS) acvm_amd/csrc/wire_plan.hpp acvm_amd/csrc/assigned_view.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(WIRE_DEFLATE_SRCS)
tools/asan/wire_in_plan_host_test: $(WIRE_IN_SRCS) acvm_amd/csrc/wire_in_plan.hpp acvm_amd/csrc/wire_plan.hpp acvm_amd/csrc/assigned_view.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(WIRE_IN_SRCS)
tools/asan/wire_inflate_plan_host_test: tools/wire_inflate_plan_host_test.cpp $(WIRE_INFLATE_PLAN_SRCS) $(WIRE_INFLATE_HDRS)
	$(CXX) $(ASAN_FLAGS) -o $@ tools/wire_inflate_plan_host_test.cpp $(WIRE_INFLATE_PLAN_SRCS)
tools/asan/wire_inflate_host_test: tools/wire_inflate_host_test.hip acvm_amd/csrc/wire_inflate.hpp acvm_amd/csrc/wire_encode.hpp $(WIRE_INFLATE_PLAN_SRCS) $(WIRE_INFLATE_HDRS)
	$(HIPCC) --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tools/wire_inflate_host_test.hip $(WIRE_INFLATE_PLAN_SRCS)
tools/asan/assigned_view_host_test: tools/assigned_view_host_test.cpp acvm_amd/csrc/assigned_view.hpp
	$(CXX) $(ASAN_FLAGS) -o $@ tools/assigned_view_host_test.cpp
BRILLIG_RETRY_SRCS = tools/brillig_retry_plan_host_test.cpp acvm_amd/csrc/brillig_retry_plan.cpp
tools/asan/brillig_retry_plan_host_test: $(BRILLIG_RETRY_SRCS) acvm_amd/csrc/brillig_retry_plan.hpp acvm_amd/csrc/brillig_resume.hpp
	$(CXX) $(ASAN_FLAGS) -o $@ $(BRILLIG_RETRY_SRCS)
tools/asan/brillig_resume_host_test: tools/brillig_resume_host_test.hip acvm_amd/csrc/brillig_resume.hpp
	$(HIPCC) --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tools/brillig_resume_host_test.hip
WIRE_PACK_SRCS = tools/wire_pack_plan_host_test.cpp acvm_amd/csrc/wire_pack_plan.cpp acvm_amd/csrc/wire_plan.cpp
tools/asan/wire_pack_plan_host_test: $(WIRE_PACK_SRCS) acvm_amd/csrc/wire_pack_plan.hpp acvm_amd/csrc/wire_plan.hpp acvm_amd/csrc/assigned_view.hpp include/acvm_amd.h
	$(CXX) $(ASAN_FLAGS) -o $@ $(WIRE_PACK_SRCS)
tools/asan/wire_repitch_host_test: tools/wire_repitch_host_test.hip acvm_amd/csrc/wire_repitch.hpp acvm_amd/csrc/wire_encode.hpp
	$(HIPCC) --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o $@ tools/wire_repitch_host_test.hip
.PHONY: asan
