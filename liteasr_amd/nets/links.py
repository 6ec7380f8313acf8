"""What the encoder layers' autograd nodes hand each other across their boundaries (host side
only: no kernel is launched here, and nothing here needs a GPU).

The encoder stack is one autograd node per layer (nets/functional.py ConformerLayerFn /
TransformerLayerFn), and neighbouring nodes cooperate:

  * forward (FUSED_LN2): a layer's final norm also computes the first norm of the layer above;
  * backward (LN2_BWD_CHAIN): a layer's first-norm backward also runs the final-norm backward
    of the layer below, and RETURNS that layer's dx4 to autograd in place of its own input
    gradient; the branch gradient gb that came out of the same launch travels beside it;
  * parameter-gradient reductions (LAYER_RED_HOLD) stay queued until the lowest layer of the
    backward segment;
  * the positional projections are computed once for all layers.

The model builds one LayerLink per layer for every forward (``LayerLink.stack``) and publishes
them as ``env.links``; a node finds its own with ``env.links[layer]``.  ``env.links = None`` is
a standalone node: no chaining, the layer projects its own positions, its reductions launch at
the end of the node.  Fresh records each forward: nothing survives into the next step."""


class LayerLink:
    """layer, below, above: the layer module and the neighbouring records (None at the ends).
    floor: the lowest layer of its backward segment (layer 0, or a graph-segment cut lies between
    it and the layer below); its node launches the reductions the layers above left queued.
    pos_p: the layer's slice of the batched positional projection, or None (it projects itself)."""

    __slots__ = ("layer", "below", "above", "floor", "pos_p", "_fwd", "_bwd")

    def __init__(self, layer, below=None, floor=True, pos_p=None):
        self.layer, self.below, self.above, self.floor, self.pos_p = layer, below, None, floor, pos_p
        self._fwd = self._bwd = None
        if below is not None:
            below.above = self

    @staticmethod
    def stack(layers, cuts=(), pos_p=None):
        """{layer: record} of a layer stack, bottom up.  cuts: the backward-segment cuts (j: before
        layer j; values outside the stack are other cuts of the model and do not matter here)."""
        links, below = {}, None
        for j, layer in enumerate(layers):
            links[layer] = below = LayerLink(layer, below, j == 0 or j in cuts, pos_p[j] if pos_p else None)
        return links

    # ---- forward: the layer below deposits this layer's first norm
    def give_first_norm(self, x5, z, mean, rstd, x4, mf, rf):
        """z, mean, rstd: this layer's first norm of x5, the output of the layer below; x4, mf,
        rf: that layer's final-norm input and statistics, which the chained backward needs."""
        self._fwd = (x5, z, mean, rstd, x4, mf, rf)

    def take_first_norm(self, x0):
        """(z, mean, rstd, (x4, mf, rf)) when a deposit was computed from x0's storage (a cut's
        detached leaf still is that storage), and the deposit is gone; else None."""
        f = self._fwd
        if f is None or f[0].data_ptr() != x0.data_ptr():
            return None
        self._fwd = None
        return f[1], f[2], f[3], f[4:]

    # ---- backward: the layer above deposits this layer's dx4 (the tensor it returns) and gb
    def give_final_grad(self, dx4, gb):
        self._bwd = (dx4, gb)

    def take_final_grad(self, dx5):
        """gb when the layer above deposited (the incoming dx5 is then this layer's dx4), None
        when it did not; either way the deposit is gone.  Only the very tensor that was produced
        is accepted: autograd hands a single consumer's gradient on without a copy (between two
        nodes, and through autograd.grad / autograd.backward at a segment cut), so anything else
        -- a hook's result, a second consumer's sum, a copy -- is not dx4 and is refused."""
        b, self._bwd = self._bwd, None
        if b is None:
            return None
        if (dx5.data_ptr(), dx5.shape, dx5.dtype) != (b[0].data_ptr(), b[0].shape, b[0].dtype):
            raise RuntimeError("ConformerLayerFn: the chained final-norm gradient did not arrive as produced")
        return b[1]

    @staticmethod
    def leftover(links):
        """Raises when a backward deposit was never collected: the layer it was meant for did not
        run, yet its dx4 went down the graph as if it were an input gradient."""
        if any(link._bwd is not None for link in (links or {}).values()):
            raise RuntimeError("ConformerLayerFn: a chained final-norm gradient was never collected")
