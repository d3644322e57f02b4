# same-box A/B of the training step (tools/train_probe.py, B = 64): forward projections and dX on the own kernels (the "train" rows of
# zigma_amd/routing.py) vs on the library (those rows disabled)
for rnd in 1 2; do
for knobs in "" "routing.DISABLED=train.ws+train.ws128+train.tiled"; do
  echo -n "== ZIGMA_KNOBS=$knobs: "
  B=64 ZIGMA_KNOBS=$knobs python tools/train_probe.py 2>/dev/null | tail -1 | cut -c1-260
done
done
