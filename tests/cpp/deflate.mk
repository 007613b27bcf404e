# AddressSanitizer + UndefinedBehaviorSanitizer build of the lossless tile codec's scalar encoder and the lossless host writer
# (csrc/deflate_rle.hpp and tiff_pyramid.hpp through image_io.cpp; no HIP, plain g++):
#   make -C tests/cpp -f deflate.mk   -> build/san_deflate, driven by tests/test_deflate_sanitizers.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
HOST  := $(SRC)/jpeg_decode.cpp $(SRC)/png_decode.cpp $(SRC)/image_io.cpp
HDRS  := $(SRC)/image_io.hpp $(SRC)/jpeg_decode.hpp $(SRC)/jpeg_encode.hpp $(SRC)/deflate_rle.hpp $(SRC)/tiff_pyramid.hpp $(ROOT)/include/pifusion.h
FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -I$(SRC) -I$(ROOT)/include
OUT   ?= build

$(OUT)/san_deflate: san_deflate.cpp $(HOST) $(HDRS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all san_deflate.cpp $(HOST) -o $@ -lz -lpthread
