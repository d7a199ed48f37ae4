#!/usr/bin/env bash
# Per-kernel register / spill / scratch usage of the render and ray-query kernels (device compile
# only); KERNELS=<awk regex> picks others, e.g. KERNELS='k_rb_|k_pc_|k_fit_cost' for the rebuild's.
# usage: tools/resource_usage.sh [extra hipcc flags...]
set -eu
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -c \
  -Rpass-analysis=kernel-resource-usage "$@" -o /tmp/myrt_ru.o myraytracer_amd/csrc/render.hip 2>&1 |
  sed -n 's/.*remark: *//p' | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//' |
  awk -v pick="${KERNELS:-render_kernel|render_full|k_query|k_ray_bounds}" \
      '/^Function Name: /{show=($3 ~ pick); if (show) print $3; next}
       show && /^(TotalSGPRs|VGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)/{printf "    %s\n", $0}'
