# Per-kernel register / spill / scratch / LDS usage of liblnw's kernels in lnw_kernels.hip
# (gfx950), from the compiler's kernel-resource-usage remarks:
#   bash tools/resource_usage.sh        the step kernels
#   bash tools/resource_usage.sh all    every kernel of the file
cd "$(dirname "$0")/.." || exit 1
C=littoral-naval-warfare-marl_amd/csrc
KEEP="step_kernel|step_group"
[ "$1" = all ] && KEEP="."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero \
  -Iinclude -I${SRC:-$C} --cuda-device-only -c ${SRC:-$C}/lnw_kernels.hip -o /tmp/lnw_ru.o \
  -Rpass-analysis=kernel-resource-usage 2>&1 \
  | grep -E "Function Name|TotalSGPRs:|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs Spill|LDS Size" \
  | sed -e 's/.*remark: //' | paste - - - - - - - - | sed -e 's/\[-Rpass-analysis=kernel-resource-usage\]//g' | grep -E "$KEEP"
