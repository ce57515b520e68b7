#!/bin/bash
# class-2 crops of the certified argmax (TTUP_CERT_SMALL=0: off; read once per process): the bench regimes on ONE box, alternating
#   tools/crop_ab.sh [OUT_DIR]     (bench lines and their stderr go to OUT_DIR, default bench_crop_ab/)
OUT=${1:-bench_crop_ab}; mkdir -p "$OUT"
for sm in 0 1 0 1; do
  TTUP_CERT_SMALL=$sm python bench.py --full --no-cpu-baseline > "$OUT/bench_small$sm.json" 2> "$OUT/bench_small$sm.err"
  python -c "
import json
d=json.load(open('$OUT/bench_small$sm.json'))
n=d['noise_weights_fps']; v=d['varied_content_fps']
print('small $sm', d['value'], 'varied', v['value'], v['crops_per_heatmap'], 'exact', d['exact_windows_fps']['value'], 'noise', n['value'], n['crops_per_heatmap'], n.get('small_core_crop_share'), v.get('small_core_crop_share'), d['exact_windows_fps'].get('small_core_crop_share'), 'cnn', d['cnn_only_fps']['value'], 'hub', d['hub_clip_fps']['value'], d['hub_clip_fps_256']['value'])
"
done
