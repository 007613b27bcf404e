# AddressSanitizer + UndefinedBehaviorSanitizer build of the check of the cull's bounds with the pyramid's slack (csrc/frame_plan.hpp; no
# HIP, plain g++; -ffp-contract=off like the library):
#   make -C tests/cpp -f cull_slack.mk   -> build/cull_slack_check, driven by tests/test_cull_slack.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
OUT   ?= build

$(OUT)/cull_slack_check: cull_slack_check.cpp $(SRC)/frame_plan.hpp $(SRC)/plan_limits.hpp
	mkdir -p $(OUT)
	$(CXX) -std=c++17 -O1 -g -ffp-contract=off -fno-omit-frame-pointer -Wall -I$(SRC) -fsanitize=address,undefined -fno-sanitize-recover=all cull_slack_check.cpp -o $@
