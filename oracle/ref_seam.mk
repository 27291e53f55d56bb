# Boundary test: the reference's core/krylov_decomposition.f, read from $(REF) at build time and compiled
# UNCHANGED (fixed form, -fdefault-real-8 as Nek5000's -r8), against host/ref_seam/krylov_subspace_hip.f90, into _ref/seam/
# (git-ignored, with the other builds of reference code).  The binary finds the library relative to itself.
# host/ref_seam/include/SIZE, TOTAL are stand-ins that declare nid / mstep / ifres only: this is a test of the seam, not an oracle.
#     make -C oracle -f ref_seam.mk REF=<the reference's tree>        (oracle/build_ref.py: build_seam)
ifeq ($(REF),)
$(error REF=<the reference's tree> is required)
endif
HOST   := ../host
SEAM   := _ref/seam
LIBDIR := $(abspath ../nekstab_amd/lib)
$(SEAM)/ref_seam_driver: $(HOST)/nekstab_hip_mod.f90 $(HOST)/ref_seam/krylov_subspace_hip.f90 $(HOST)/ref_seam/nek_support.f90 $(HOST)/ref_seam/seam_driver.f90 $(REF)/core/krylov_decomposition.f
	mkdir -p $(SEAM)
	flang -O2 -c -module-dir $(SEAM) -o $(SEAM)/nekstab_hip_mod.o $(HOST)/nekstab_hip_mod.f90
	flang -O2 -c -module-dir $(SEAM) -o $(SEAM)/krylov_subspace_hip.o $(HOST)/ref_seam/krylov_subspace_hip.f90
	flang -O2 -c -o $(SEAM)/nek_support.o $(HOST)/ref_seam/nek_support.f90
	flang -O2 -c -fdefault-real-8 -ffixed-line-length=none -I$(HOST)/ref_seam/include -I$(SEAM) -o $(SEAM)/krylov_decomposition.o $(REF)/core/krylov_decomposition.f
	flang -O2 -c -module-dir $(SEAM) -o $(SEAM)/seam_driver.o $(HOST)/ref_seam/seam_driver.f90
	flang -O2 -o $@ $(SEAM)/seam_driver.o $(SEAM)/krylov_decomposition.o $(SEAM)/krylov_subspace_hip.o $(SEAM)/nek_support.o $(SEAM)/nekstab_hip_mod.o -L$(LIBDIR) -lnekstab_hip -Wl,-rpath,'$$ORIGIN/../../../nekstab_amd/lib'
