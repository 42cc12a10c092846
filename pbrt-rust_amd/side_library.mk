# The recipe of an integrator library beside libmi355pt.so -- libmi355$(NAME).so from $(NAME)_render.hip + $(NAME)_kernels.h (include/mi355$(NAME).h), hand-written HIP
# for gfx950 (MI355X). Included by the library directory's Makefile, which sets NAME. The library links against ../csrc/libmi355pt.so (scenes, workspace, traversal,
# camera and film kernels, render frame) and exports only what its exports.map names (-fvisibility=hidden), so that none of its symbols can interpose one of libmi355pt's.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS = -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-result -Wno-unused-value -fvisibility=hidden $(EXTRA_HIPFLAGS)
CSRC_HDRS = $(wildcard ../csrc/*.h) ../../include/mi355pt.h ../../include/pt_noise_perm.h
SIDE_HDRS = $(wildcard ../side/*.h)   # what the side libraries share among themselves

libmi355$(NAME).so: $(NAME)_render.o exports.map ../csrc/libmi355pt.so
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(NAME)_render.o -L../csrc -lmi355pt -Wl,-rpath,'$$ORIGIN/../csrc' -Wl,--version-script=exports.map

$(NAME)_render.o: $(NAME)_render.hip $(NAME)_kernels.h ../../include/mi355$(NAME).h $(CSRC_HDRS) $(SIDE_HDRS)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $(NAME)_render.hip

clean:
	rm -f *.o libmi355$(NAME).so
.PHONY: clean
