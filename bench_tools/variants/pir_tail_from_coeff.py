COMPILE = ["pir_api.cpp"]
DESCRIPTION = "the chunk loop's first remaining dimension from Coeff-form dim-0 results, as the reference does it: inverse transform, lift with the copy of the Q rows, forward transform of all rows (production: the Eval-form Q rows are kept)"
EDITS = [("pir_api.cpp", "        const bool in_eval = heamd::kDim0ResultsStayEval<W>;\n",
          "        const bool in_eval = false;\n")]
