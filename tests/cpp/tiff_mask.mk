# AddressSanitizer + UndefinedBehaviorSanitizer build of the host writer of the masked pyramid TIFF (csrc/tiff_pyramid.hpp through
# image_io.cpp's pf_tiff_write_bgr_masked; no HIP, plain g++):   make -C tests/cpp -f tiff_mask.mk   -> build/san_tiff_mask, driven
# by tests/test_tiff_mask.py
CXX   ?= g++
ROOT  := ../..
SRC   := $(ROOT)/pi-slam-fusion_amd/csrc
HOST  := $(SRC)/jpeg_decode.cpp $(SRC)/png_decode.cpp $(SRC)/image_io.cpp
HDRS  := $(SRC)/image_io.hpp $(SRC)/jpeg_decode.hpp $(SRC)/jpeg_encode.hpp $(SRC)/tiff_pyramid.hpp $(ROOT)/include/pifusion.h
FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -I$(SRC) -I$(ROOT)/include
OUT   ?= build

$(OUT)/san_tiff_mask: san_tiff_mask.cpp $(HOST) $(HDRS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all san_tiff_mask.cpp $(HOST) -o $@ -lz -lpthread
