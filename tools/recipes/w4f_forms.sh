#!/bin/bash
# F(4x4,3x3) OUTPUT transform alone, every form the step launches x 128 / 256 / 512 channels: the one-pixel-at-a-time kernel against the
# two-phase kernel and its timing ablations (rocprofv3 --kernel-trace over tools/wino4f_probe.py forms).  The table goes to stdout.
R=$(cd "$(dirname "$0")/../.." && pwd)
O=$(mktemp -d) || exit 1
( cd $O && export TMPDIR=$O && rocprofv3 --kernel-trace -d $O -o kt -- python $R/tools/wino4f_probe.py forms $O/manifest.json 32 29 > $O/kt.out 2> $O/kt.err ) || { tail -20 $O/kt.err; rm -rf $O; exit 1; }
DB=$(find $O -name "kt_results.db")
python $R/tools/wino4f_trace.py forms $DB $O/manifest.json
rc=$?
rm -rf $O
exit $rc
