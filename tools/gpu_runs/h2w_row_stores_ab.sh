# same-box A/B of the Winograd split-precision convolution before / after a change of its header (conv3d_wino_h2.h), against a PREVIOUS build kept out of git.
# Built beforehand, in the build container (F = the flags of tools/ubench/h2w_variants.hip's first lines; <prev> = a checkout of the previous commit, `git worktree add`):
#   (cd <prev> && python -m monai_amd.build) && mkdir -p tools/ubench/_old variants && cp <prev>/monai_amd/csrc/libmonai_amd.so tools/ubench/_old/
#   hipcc $F -Iinclude -I<prev>/monai_amd/csrc tools/ubench/h2w_variants.hip -o tools/ubench/_old/h2wv       # PREV (default tools/ubench/_old): library + harness
#   hipcc $F -Iinclude -Imonai_amd/csrc tools/ubench/h2w_variants.hip -o variants/h2wv && python -m monai_amd.build      # NEW (default variants): harness; this tree's library
# Parts [PARTS="bits pmc layers trace headline" by default], everything under $O (default build/h2w_rows):
#   bits      bench.py --dump-outputs of previous, previous, this tree: the dumps byte for byte (two previous runs first: the comparison means something only if they agree)
#   pmc       counters of the standalone harness, passes of their own with only the kernel trace beside them
#   layers    tools/h2w_bench.py alternating     trace   kernel traces of the headline     headline   three runs each, alternating
set -o pipefail
export TMPDIR=/tmp
R=$PWD; PREV=$R/${PREV:-tools/ubench/_old}; NEW=$R/${NEW:-variants}
O=${O:-$R/build/h2w_rows}; mkdir -p $O
side_env() { case $1 in P*) export MONAI_AMD_LIB=$PREV/libmonai_amd.so;; *) unset MONAI_AMD_LIB;; esac; }
for part in ${PARTS:-bits pmc layers trace headline}; do
  case $part in
  bits)
    : > $O/bits.txt
    for tag in P1 P2 B1; do
      side_env $tag
      timeout -k 10 170 python bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs $O/dump_$tag > $O/dump_$tag.json 2> $O/dump_$tag.err || { tail -20 $O/dump_$tag.err; exit 1; }
      echo "$tag $(tail -1 $O/dump_$tag.json | python -c "import json,sys; print(repr(json.loads(sys.stdin.readline()).get('checksum')))")" | tee -a $O/bits.txt
    done
    for f in $O/dump_P1/*.npy; do
      b=$(basename $f)
      cmp $f $O/dump_P2/$b && echo "previous == previous: $b" || echo "PREVIOUS RUNS DIFFER: $b"
      cmp $f $O/dump_B1/$b && echo "previous == this tree: $b" || echo "THIS TREE DIFFERS: $b"
    done | tee -a $O/bits.txt
    rm -rf $O/dump_P1 $O/dump_P2 $O/dump_B1
    if grep -q DIFFER $O/bits.txt; then exit 1; fi;;
  pmc)
    : > $O/pmc.txt
    for side in $PREV $NEW; do
      for C in "TCP_TCC_WRITE_REQ_sum TCP_TCC_READ_REQ_sum TCC_REQ_sum TA_BUSY_avr TCP_PENDING_STALL_CYCLES_sum" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_BUSY_CYCLES"; do
        rm -rf $O/p
        ( cd /tmp && timeout -k 10 200 rocprofv3 --kernel-trace --pmc $C -d $O/p -o w -- $side/h2wv pmc > $O/run.log 2>&1 ) || { tail -20 $O/run.log; exit 1; }
        echo "== $side: $C" >> $O/pmc.txt
        find $O/p -name "*.db" | head -1 | xargs -I{} python $R/tools/pmc_stats.py {} "%h2w_kernel%" >> $O/pmc.txt 2>&1
        tail -1 $O/run.log >> $O/pmc.txt
      done
    done
    rm -rf $O/p; cat $O/pmc.txt;;
  layers)
    for tag in P1 B1 P2 B2; do
      side_env $tag
      timeout -k 10 200 python tools/h2w_bench.py > $O/h2w_bench_$tag.json 2> $O/h2w_bench_$tag.err || { tail -20 $O/h2w_bench_$tag.err; exit 1; }
    done;;
  trace)
    for tag in P B; do
      side_env $tag; rm -rf $O/prof
      timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python bench.py --gpus 1 --steps 7 --warmup 2 > $O/traced_$tag.json 2> $O/trace_$tag.err || { tail -20 $O/trace_$tag.err; exit 1; }
      find $O/prof -name "*.db" | head -1 | xargs -I{} python tools/rocpd_stats.py {} > $O/kernel_trace_stats_$tag.txt 2>&1
      rm -rf $O/prof; head -14 $O/kernel_trace_stats_$tag.txt | cut -c1-200
    done;;
  headline)
    for tag in P1 B1 P2 B2 P3 B3; do
      side_env $tag
      timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 > $O/bench_$tag.json 2> $O/bench_$tag.err || { tail -20 $O/bench_$tag.err; exit 1; }
      echo "$tag $(tail -1 $O/bench_$tag.json | cut -c1-160)" | tee -a $O/headline.txt
    done;;
  esac
done
