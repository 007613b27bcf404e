# AddressSanitizer + UndefinedBehaviorSanitizer build of the host JPEG encoder (csrc/jpeg_encode.hpp through image_io.cpp's entry
# points; no HIP, plain g++):   make -C tests/cpp -f jpeg_encode.mk   -> build/san_jpeg_encode, driven by tests/test_jpeg_encode.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
HOST  := $(SRC)/jpeg_decode.cpp $(SRC)/png_decode.cpp $(SRC)/image_io.cpp
HDRS  := $(SRC)/jpeg_decode.hpp $(SRC)/jpeg_encode.hpp $(ROOT)/include/pifusion.h
FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -I$(SRC) -I$(ROOT)/include
OUT   ?= build

$(OUT)/san_jpeg_encode: san_jpeg_encode.cpp $(HOST) $(HDRS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all san_jpeg_encode.cpp $(HOST) -o $@ -lz -lpthread
