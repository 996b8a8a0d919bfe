#!/bin/bash
# usage: tools/kasm.sh <file.hip> -- the gfx950 device assembly of one source on stdout, with build.py's flags.  Two versions of a
# kernel compare with one diff: -fuse-cuid=none keeps the __hip_cuid_<hash> symbol, which hashes the input, out of the output.
/opt/rocm/bin/hipcc --offload-arch=gfx950:xnack- -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -Wno-unused-value \
  --cuda-device-only -S -fuse-cuid=none "$1" -o -
