# AddressSanitizer + UndefinedBehaviorSanitizer build of the host raw-frame converter (csrc/raw_convert.hpp, header only; no HIP, plain g++):
#   make -C tests/cpp -f raw_convert.mk   -> build/san_raw_convert, driven by tests/test_raw_sanitizers.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
HDRS  := $(SRC)/raw_convert.hpp $(ROOT)/include/pifusion.h
FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -I$(SRC) -I$(ROOT)/include
OUT   ?= build

$(OUT)/san_raw_convert: san_raw_convert.cpp $(HDRS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all san_raw_convert.cpp -o $@
