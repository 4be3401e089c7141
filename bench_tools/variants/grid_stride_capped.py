COMPILE = ["poly_kernels.hip", "galois_kernels.hip", "rns_kernels.hip", "copy_kernels.hip"]
DESCRIPTION = "the element-wise kernels on 256 x 8 (rns_kernels: 256 x 16) workgroups walking their items with a grid-stride loop, as until round 6 (production: one workgroup per 256 items)"
_OLD = "inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads); }"
EDITS = [("poly_kernels.hip", _OLD, "inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads, 256 * 8); }"),
         ("galois_kernels.hip", _OLD, "inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads, 256 * 8); }"),
         ("rns_kernels.hip", _OLD, "inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads, 256 * 16); }"),
         ("copy_kernels.hip", _OLD, "inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads, 256 * 8); }")]
