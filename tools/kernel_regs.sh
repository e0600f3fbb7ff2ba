#!/bin/bash
# VGPR / scratch usage of every fused-kernel instantiation: tools/kernel_regs.sh [qnet_fused|qnet_fused_split|qnet_fused_jobs|qnet_fused_step]
# (a forward kernel's name ends in Lb0 = the plain form, Lb1 = the job-table form)
# Any other source file with the kernel-name pattern to keep as second argument: tools/kernel_regs.sh env rollout_ply
f=${1:-qnet_fused}
pat=${2:-qnet_}
cd "$(dirname "$0")/../gnn_hex_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -c -Rpass-analysis=kernel-resource-usage -o /tmp/$f.regs.o $f.hip 2>&1 |
  awk '/Function Name:/ {name=$0; sub(/.*Function Name: /,"",name); sub(/ \[.*/,"",name)} / VGPRs:/ {v=$0; sub(/.* VGPRs: /,"",v); sub(/ \[.*/,"",v)} /ScratchSize/ {s=$0; sub(/.*: /,"",s); sub(/ \[.*/,"",s); print name, "vgprs", v, "scratch", s}' | grep "$pat" | sed 's/_ZN6hexgnn1[56]//; s/EEEv[A-Za-z0-9_]*//'
