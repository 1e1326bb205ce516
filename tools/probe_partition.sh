#!/bin/bash
# Does the gpurun box let one MI355X appear as several devices (compute partitioning: CPX exposes
# the 8 XCDs as 8 devices), so that RCCL could run with > 1 real rank?  Read-only probes: the partition
# mode is reported, never changed.  Every step under its own timeout.
set -u
O=${GRAFT_REPO_ROOT:-/root/repo}/gpurun_out/partition_probe
mkdir -p $O
{
echo "== devices as seen"; timeout 60 rocminfo | grep -E "Marketing Name|gfx9|Compute Unit" | head -20
echo "== rocm-smi --showcomputepartition / --showmemorypartition"
timeout 60 rocm-smi --showcomputepartition 2>&1 | tail -8
timeout 60 rocm-smi --showmemorypartition 2>&1 | tail -8
echo "== amd-smi partition"
timeout 60 amd-smi partition 2>&1 | head -40
echo "== sysfs"
for f in /sys/class/drm/card*/device/current_compute_partition /sys/class/drm/card*/device/available_compute_partition /sys/class/drm/card*/device/current_memory_partition; do
  [ -e "$f" ] && { echo "$f: $(cat $f 2>&1)"; ls -l $f; }
done
echo "== torch device count"; timeout 120 python -c "import torch; print(torch.cuda.device_count())"
NDEV=$(timeout 120 python -c "import torch; print(torch.cuda.device_count())" 2>/dev/null | tail -1)
if [ "${NDEV:-1}" -gt 1 ]; then
  echo "== $NDEV devices: the multi-device RCCL tests"
  cd ${GRAFT_REPO_ROOT:-/root/repo}
  timeout 900 python -m pytest tests/test_gpu_fullsize.py -q -x -k "rccl_on_real_devices" 2>&1 | tail -15
  timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 20 --warmup 5 --colpart-vars 4096 2>&1 | tail -5
fi
} > $O/probe.log 2>&1
cat $O/probe.log
