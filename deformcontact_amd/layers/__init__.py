"""One module per layer family: a launcher per C entry, the autograd Functions, and the validating public function.

``deformcontact_amd.ops`` re-exports the public names (call them as ``ops.<name>``) and the launchers that the kernel
tests call by name; everything else is reached here.  A module reads a run-time switch as ``ops.NAME`` at call time -
the switches all live in ``ops.py`` - and imports only from ``ops``, ``_host`` and the layer modules below it: ``gnn``
<- ``gat_heads`` <- ``gatv2``, ``transformer``; ``sage`` <- ``gine``, ``edge`` <- ``pointnet``; ``gnn``, ``sage`` <-
``gmm`` <- ``spline``; ``cheb``."""
