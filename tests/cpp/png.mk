# AddressSanitizer + UndefinedBehaviorSanitizer build of the scalar encoder of the PNG of save_png, its checksums and the host writer
# (csrc/png_encode.hpp through image_io.cpp; no HIP, plain g++):
#   make -C tests/cpp -f png.mk   -> build/san_png, driven by tests/test_png_sanitizers.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
HOST  := $(SRC)/jpeg_decode.cpp $(SRC)/png_decode.cpp $(SRC)/image_io.cpp
HDRS  := $(SRC)/image_io.hpp $(SRC)/jpeg_decode.hpp $(SRC)/jpeg_encode.hpp $(SRC)/deflate_rle.hpp $(SRC)/png_encode.hpp $(SRC)/tiff_pyramid.hpp $(ROOT)/include/pifusion.h
FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -I$(SRC) -I$(ROOT)/include
OUT   ?= build

$(OUT)/san_png: san_png.cpp $(HOST) $(HDRS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all san_png.cpp $(HOST) -o $@ -lz -lpthread
