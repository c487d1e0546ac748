# register / LDS / spill summary of every kernel of ccsx_kernels.hip, ccsx_train.hip, ccsx_refine.hip, ccsx_deflate.hip, ccsx_barcode.hip, ccsx_segment.hip, ccsx_cdna.hip, ccsx_represent.hip, ccsx_dup.hip and ccsx_cell.hip (with the sort it instantiates; no GPU needed): bash tools/kres.sh [extra hipcc flags]
cd "$(dirname "$0")/.."
for src in ccsx_kernels.hip ccsx_train.hip ccsx_refine.hip ccsx_deflate.hip ccsx_barcode.hip ccsx_segment.hip ccsx_cdna.hip ccsx_represent.hip ccsx_dup.hip ccsx_cell.hip; do
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-value -fno-slp-vectorize -falign-loops=64 \
  -Iinclude -Iccs_amd/csrc "$@" -Rpass-analysis=kernel-resource-usage -c ccs_amd/csrc/$src -o /tmp/kres.o 2>&1 |
  grep -E "Function Name|VGPRs:|SGPRs Spill|VGPRs Spill|ScratchSize|LDS Size|Occupancy" | sed 's/.*remark: //' | paste - - - - - - - | sed 's/\[-Rpass-analysis=kernel-resource-usage\]//g'
done
