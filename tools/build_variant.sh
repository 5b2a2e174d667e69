#!/bin/bash
# diagnostic builds of the library with extra -D flags: tools/build_variant.sh <name> <flags...>  -> mamdr_amd/build/variants/lib<name>.so
# (the sources and flags are those of the product build: mamdr_amd/build.py)
cd "$(dirname "$0")/.." && exec python3 -m mamdr_amd.build --variant "$@"
